/*
 * mmgclip_hip.h — C ABI of libmmgclip_hip.so: the hand-written gfx950 (MI355X / CDNA4) kernels behind
 * mmg-clip's contrastive-training hot path.
 *
 * The reference (abdel-habib/mmg-clip) has no FFI of its own: its hot path is Python calling ATen.  Each entry
 * below therefore cites the reference Python call site (path:line in the reference tree) whose arithmetic it
 * replaces; INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch allocations in this repo); nothing is
 *     allocated, freed or retained by the library; no global state besides a thread-local error string (and the opt-in
 *     kernel-name note of the diagnostics below);
 *   - `stream` is a hipStream_t passed as void* (PyTorch's current stream); every call is asynchronous on it
 *     and safe to capture into a hipGraph;
 *   - matrices are row-major; `ld*` are leading dimensions in ELEMENTS;
 *   - bf16 tensors are passed as `void*` (raw 16-bit payload), fp32 as `float*`, token ids as `long long*`;
 *   - return value: 0 = launched, non-zero = rejected (bad shape / null pointer / launch error) and
 *     mmg_last_error() holds the reason.  Host wrappers raise on non-zero.
 *
 * This header is the single source of truth: mmgclip/_hip.py parses it to build the ctypes prototypes and
 * tests/test_abi.py checks that the library exports every symbol declared here.
 */
#ifndef MMGCLIP_HIP_H
#define MMGCLIP_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mmg_stream_t; /* hipStream_t */

/* ---- library probe ------------------------------------------------------------------------------------ */
int mmg_abi_version(void);
const char* mmg_last_error(void);
const char* mmg_target_arch(void);
int mmg_device_cu_count(void);
/* Diagnostics for the measurement leg (bench.py `roofline`, mmgclip/profile.py): while notes are on, every dispatcher records the
 * name of the kernel instantiation it launches - spelled as rocprofv3's kernel trace spells it, e.g.
 * "gemm_nt_kernel<256, 256, 64, 4, 2, 0>" - and mmg_last_kernel() returns the calling thread's last one ("" when none).  No
 * reference counterpart: the reference has no kernels of its own to name. */
int mmg_set_kernel_notes(int on);
const char* mmg_last_kernel(void);
/* What a GEMM entry point WOULD launch for a shape, without launching: the plan its host layer makes (csrc/gemm_plan.h) as text -
 * the exact mmg_last_kernel() spelling, then " grid=(x,y) block=T lds=B" (B = dynamic LDS bytes); the weight-gradient ops continue
 * with " chunks=.. rows=.. xcd=.. swapped=.." (split of the reduction, rows per chunk, XCD grouping mode, operands exchanged) and the
 * 8-bit ones with " split=..".  op: 0 mmg_gemm_nt_bf16, 1 mmg_gemm_nt_fp8, 2 / 3 mmg_gemm_nt_fp8_bwd with e5m2 / e4m3 A,
 * 4 mmg_gemm_tn_bf16 (N = N1, K = N2), 5 / 6 mmg_gemm_tn_fp8 with e5m2 / e4m3 A (N = N1, K = N2); contiguous operands, no epilogue.
 * cus: CU count the plan is made for, 0 = the current device's.  Honours the same environment knobs as the entry points.  A shape the
 * entry point would reject gives "" and sets mmg_last_error() to that entry point's message.  The string belongs to the calling thread
 * and is valid until its next call.  No reference counterpart (diagnostics; tests/test_gemm_plan_cpu.py pins kernel selection with it).
 * Additive entry point: it came without an ABI version step (mmg_abi_version() stays 5). */
const char* mmg_gemm_plan(int op, int M, int N, int K, int cus);

/* ---- contrastive head (fp32, f32-input MFMA) ------------------------------------------------------------ */

/* y = x / ||x||_2 per row, no epsilon; norm[r] = ||x_r||.
 * Replaces mmgclip/networks/mmgclip_model.py:128-129. */
int mmg_l2norm_fwd(const float* x, float* y, float* norm, int rows, int D, mmg_stream_t stream);
/* dx = (dy - y <y,dy>) / norm   (autograd of the line above) */
int mmg_l2norm_bwd(const float* y, const float* norm, const float* dy, float* dx, int rows, int D,
                   mmg_stream_t stream);

/* For the n_loc local rows X against the N gathered rows Y (both L2-normalised, [.,D] fp32):
 *   lse[i] = logsumexp_j( s <X_i,Y_j> ),  pos[i] = s <X_i, Y_{diag_off+i}>,  s = *scale
 * and, when logits != NULL, logits[i*ldl + j] = s <X_i,Y_j>.
 * Replaces mmgclip/networks/mmgclip_model.py:132-136 (logit_scale * I @ T.t()) fused with the
 * log-softmax of mmgclip/loss/losses.py:40-41.  D % 32 == 0, D <= 1024. */
int mmg_clip_rows_fwd(const float* X, const float* Y, const float* scale, int n_loc, int N, int D, int diag_off,
                      float* lse, float* pos, float* logits, int ldl, mmg_stream_t stream);

/* Gradient of the symmetric cross-entropy w.r.t. the local rows, without materialising logits:
 *   g_ij = coef * gout * ( exp(z_ij - lse_row[i]) + exp(z_ij - lse_col[j]) - 2 [j == diag_off+i] )
 *   dX[i,:] = s * sum_j g_ij Y[j,:]        dscale += sum_ij g_ij <X_i,Y_j>   (dscale may be NULL)
 * lse_row: [n_loc] row log-sum-exps of this block; lse_col: [N] log-sum-exps of the transposed problem
 * (all ranks').  gout: device scalar (NULL = 1).  coef = 1/(2 N_global).
 * Autograd of mmgclip/loss/losses.py:39-43 through mmgclip/networks/mmgclip_model.py:135-136. */
int mmg_clip_rows_bwd_fused(const float* X, const float* Y, const float* scale, const float* lse_row,
                            const float* lse_col, const float* gout, float coef, int n_loc, int N, int D,
                            int diag_off, float* dX, float* dscale, mmg_stream_t stream);

/* Backward of materialised logits L = s X Y^T (and of the twin L' = s Y X^T):
 *   dX = s (Ga + Gb^T) Y,   dscale += <Ga + Gb^T, X Y^T>;   Ga: [n_loc,N] (ld lda), Gb: [N,n_loc] (ld ldb),
 * either may be NULL.  Autograd of mmgclip/networks/mmgclip_model.py:135-136 for arbitrary consumers. */
int mmg_clip_rows_bwd_dense(const float* X, const float* Y, const float* scale, const float* Ga, int lda,
                            const float* Gb, int ldb, int n_loc, int N, int D, float* dX, float* dscale,
                            mmg_stream_t stream);

/* Cross-entropy over materialised logits [rows,C]: lse[r] and loss_sum += weight * (lse[r] - z[r,label_r]);
 * labels NULL = arange.  Replaces F.cross_entropy at mmgclip/loss/losses.py:40-41,79-80,88-89,209-210. */
int mmg_ce_rows_fwd(const float* logits, int ld, const long long* labels, int rows, int C, float weight,
                    float* lse, float* loss_sum, mmg_stream_t stream);
/* dlogits = gout * weight * (softmax(z) - onehot(label)) */
int mmg_ce_rows_bwd(const float* logits, int ld, const long long* labels, const float* lse, const float* gout,
                    float weight, int rows, int C, float* dlogits, int ldd, mmg_stream_t stream);

/* loss += coef * ( sum_i (lse_a[i]-pos_a[i]) + sum_i (lse_b[i]-pos_b[i]) );  lse_b/pos_b may be NULL. */
int mmg_clip_loss_reduce(const float* lse_a, const float* pos_a, const float* lse_b, const float* pos_b, int n,
                         float coef, float* loss, mmg_stream_t stream);

/* ---- bf16 MFMA GEMMs (encoder towers, projection heads) -------------------------------------------------- */

/* C[M,N] = epilogue( alpha * A[M,K] B[N,K]^T + bias )   A,B bf16 row-major (K contiguous), fp32 accumulate.
 * epilogue (in this order): + bias[N];  activation by `epi`:
 *     0 none | 1 GELU(erf) (aux_out, when given, receives the pre-activation) | 2 multiply by GELU'(aux_in)
 *     (aux_out, when given, receives GELU(aux_in): the activation rebuilt for the weight-gradient GEMM)
 *     3 ReLU (aux_out as 1)  | 4 ReLU' (gate by aux_in > 0; aux_out as 2)  | 5 multiply by GELU'(aux_in) only (ABI 4: for callers that
 *     kept GELU(h) from the forward; aux_out unused) | 6 GELU(erf) whose aux_out receives GELU'(pre-activation) instead of the pre-activation
 *     (ABI 5) | 7 multiply by aux_in (ABI 5: the data gradient of a layer whose forward ran 6 / kept GELU');
 *     bf16 / e4m3 outputs of 1, 2, 5 and 6 evaluate GELU / GELU' by the polynomials of csrc/common.h (6e-4 relative), fp32 outputs by the erf form (1.5e-7);
 * then * colscale[N] (ConvNeXt layer scale), + residual[M,N] (bf16); C is bf16 (out_f32 = 0) or fp32.
 * K % 32 == 0, N % 8 == 0, leading dimensions multiples of 8.
 * Replaces nn.Linear forward / data-gradient in HF BertLayer (reference call site mmgclip/networks/encoder.py:156),
 * torchvision CNBlock + patchify convs (mmgclip/networks/encoder.py:53, mmgclip/networks/image_features.py:100)
 * and the projection heads (mmgclip/networks/projection.py:33,55-61,94-101). */
int mmg_gemm_nt_bf16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                     const float* bias, const float* colscale, const void* residual, int ldr, const void* aux_in,
                     int ldai, void* aux_out, int ldao, int epi, int out_f32, float alpha, mmg_stream_t stream);

/* Weight gradient: C[N1,N2] += alpha * A[M,N1]^T B[M,N2]  (A,B bf16; C fp32, accumulated with atomics, so the
 * caller zeroes C once per optimisation step).  colsum_a (nullable, fp32 [N1]) += alpha * column sums of A: the bias
 * gradient of the same linear, fused as one extra MFMA per fragment.  Autograd of the linears above. */
int mmg_gemm_tn_bf16(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N1, int N2,
                     float alpha, float* colsum_a, mmg_stream_t stream);

/* Bias gradient: out[n] += sum_m A[m,n]  (A bf16 [M,N]). */
int mmg_colsum_bf16(const void* A, int lda, int M, int N, float* out, mmg_stream_t stream);

/* ---- LayerNorm / elementwise / pooling / optimiser (HBM-bound) --------------------------------------------- */

/* y = (x - mean) * rstd * gamma + beta over the last dim C of bf16 x[M,C]; mean/rstd (fp32 [M], nullable) are saved
 * for the backward.  patch != 0: row m = (n,h,w) of an [n,H,W] grid is written to the 2x2-patchified position
 * row (n,h/2,w/2), columns ((h&1)*2+(w&1))*C of a [n*(H/2)*(W/2), 4C] matrix (ConvNeXt downsample: the following
 * 2x2/s2 convolution becomes a GEMM; an odd last row / column is dropped, as that convolution does).  Replaces nn.LayerNorm / LayerNorm2d of torchvision ConvNeXt and HF BERT
 * (mmgclip/networks/encoder.py:53,156) and of MLPProjectionHead (mmgclip/networks/projection.py:100). */
int mmg_layernorm_fwd(const void* x, int ldx, const float* gamma, const float* beta, float eps, void* y, int ldy,
                      float* mean, float* rstd, int M, int C, int patch, int H, int W, mmg_stream_t stream);
/* The same LayerNorm on an fp32 input row (HF BertLayer's LayerNorm(x + sublayer(x)), mmgclip/networks/encoder.py:156, with the
 * sum kept in fp32).  res (fp32 [M,C], nullable): x <- x + res IN PLACE first (x then holds the pre-LayerNorm sum the backward
 * needs).  y bf16 (operand of the next GEMM) and, when yf != NULL, an fp32 copy of it (the residual of the next sum). */
int mmg_layernorm_fwd_f32(float* x, int ldx, const float* res, int ldres, const float* gamma, const float* beta, float eps,
                          void* y, int ldy, float* yf, int ldyf, float* mean, float* rstd, int M, int C, mmg_stream_t stream);
int mmg_layernorm_bwd_f32(const void* dy, int lddy, const float* x, int ldx, const float* mean, const float* rstd,
                          const float* gamma, void* dx, int lddx, float* dgamma, float* dbeta, int M, int C,
                          const void* add, int ldadd, mmg_stream_t stream);
/* dx (bf16) and dgamma/dbeta (fp32, ACCUMULATED; both NULL to skip) given dy in the layout the forward wrote;
 * add (bf16 [M,C], nullable) is added to dx: the residual-path gradient of pre-LN transformer blocks.
 * patch != 0 with odd H and / or W (H, W > 1): dy is [(M / (H W)) (H/2) (W/2), 4C] (integer division), as mmg_layernorm_fwd wrote
 * it; the pixels of the dropped last row / column read nothing of dy, get dx = 0 (or add's row) and add nothing to dgamma / dbeta. */
int mmg_layernorm_bwd(const void* dy, int lddy, const void* x, int ldx, const float* mean, const float* rstd,
                      const float* gamma, void* dx, int lddx, float* dgamma, float* dbeta, int M, int C, int patch,
                      int H, int W, const void* add, int ldadd, mmg_stream_t stream);
/* What a LayerNorm entry point WOULD launch, without launching: the plan its host layer makes (csrc/layernorm_plan.h; all five entry
 * points validate, make one plan and launch the kernel it names) as text - the exact mmg_last_kernel() spelling, then
 * " grid=N block=256 lds=B nt=0|1" (B = dynamic LDS bytes, nt = streaming stores: outputs of 256 MiB and more, mmg_layernorm_fwd / _bwd
 * only).  door: 0 mmg_layernorm_fwd, 1 _fwd_f32, 2 _fwd_fp8, 3 _bwd, 4 _bwd_f32; res, yf (door 1), add (doors 3, 4): that optional
 * operand is given; contiguous operands, not patchified (neither changes a plan).  MMG_LN_PLAIN / MMG_LN_CH3 are honoured as by a launch.
 * A shape the entry point would reject gives "" and sets mmg_last_error() to that entry point's message.  The string belongs to the
 * calling thread and is valid until its next call; no GPU is needed.  No reference counterpart (diagnostics;
 * tests/test_layernorm_plan_cpu.py pins kernel selection with it).  Additive entry point: mmg_abi_version() stays 5. */
const char* mmg_layernorm_plan(int door, int M, int C, int res, int yf, int add);

/* y = GELU(x) elementwise, bf16, n % 8 == 0 (rebuilds the FFN activation in the backward pass). */
int mmg_gelu_fwd_bf16(const void* x, void* y, long long n, mmg_stream_t stream);
/* out = dy * act'(pre) elementwise, bf16; kind 0 = GELU(erf), 1 = ReLU, 2 = GELU(erf) by the exp-free polynomial of mmg_cnblock_bwdw; n % 8 == 0. */
int mmg_act_grad_bf16(const void* dy, const void* pre, void* out, long long n, int kind, mmg_stream_t stream);
/* dtype conversions of flat buffers */
int mmg_cast_f32_bf16(const float* x, void* y, long long n, mmg_stream_t stream);
int mmg_cast_bf16_f32(const void* x, float* y, long long n, mmg_stream_t stream);
/* dst[c,r] (bf16, ld ldd) = rowscale[r] * src[r,c] (fp32 [R,C]); rowscale nullable.  Transposed working copy of a
 * weight for the data-gradient GEMM (layer scale folded in for ConvNeXt's second linear). */
int mmg_transpose_cast_bf16(const float* src, int R, int C, const float* rowscale, void* dst, int ldd,
                            mmg_stream_t stream);

/* y[n,:] = mean over HW rows of bf16 x[n,HW,C] (fp32 out).  AdaptiveAvgPool2d(1), mmgclip/networks/encoder.py:54. */
int mmg_avgpool_fwd(const void* x, float* y, int n, int HW, int C, mmg_stream_t stream);
int mmg_avgpool_bwd(const float* dy, void* dx, int n, int HW, int C, mmg_stream_t stream);

/* Pooling the views of an exam inside the training graph: feat fp32 [V,C] (views of one study adjacent, studies in batch order) ->
 * out fp32 [S,C].  Replaces the offline torch.stack(features).mean(0) / .max(0)[0] of StudyFeatureExtractor,
 * mmgclip/networks/image_features.py:225-245.  offsets: device int32 [S+1], non-decreasing, offsets[0] = 0, offsets[S] = V; study s owns
 * rows offsets[s] .. offsets[s+1]-1, at least one.  C % 4 == 0, 8 <= C <= 3072.
 * mode 0 = mean: the rows summed in view order in fp32, one IEEE division by the count; argmax is not touched (nullable).
 * mode 1 = max: argmax int32 [S,C] receives the winner's row index into feat; the lowest row wins a tie; a NaN in any view gives NaN and
 *          its row (as torch.max).
 * Additive entry points: they came without an ABI version step (mmg_abi_version() stays 5). */
int mmg_view_pool_fwd(const float* feat, const int* offsets, float* out, int* argmax, int S, int C, int mode, mmg_stream_t stream);
/* dfeat fp32 [V,C]: mode 0: dout[s,c] / count for every view of s; mode 1: dout[s,c] where argmax[s,c] == v, else 0.  Like the forward it
 * writes every element exactly once (no atomics, no memset): bit-reproducible. */
int mmg_view_pool_bwd(const float* dout, const int* offsets, const int* argmax, float* dfeat, int S, int V, int C, int mode,
                      mmg_stream_t stream);

/* Stem im2col: fp32 pixels [n,Cin,H,W] -> bf16 rows (n,h/P,w/P) x (kh,kw,cin), zero-padded to Kp columns;
 * scale16 != 0 applies ((65535 x) - 32767.5)/32767.5 (mmgclip/networks/image_features.py:95-99).  H, W need not be
 * multiples of P: the remainder rows / columns are ignored, as a stride-P convolution does. */
int mmg_patchify(const float* img, void* out, int n, int Cin, int H, int W, int P, int Kp, int scale16,
                 mmg_stream_t stream);
/* The same rows from raw pixels, with per-image augmentation in the gather (csrc/pixel_input.hip).  img: [n,Cin,H,W] of src_kind
 * 0 = fp32 in [0,1], 1 = uint16, 2 = uint8.  geom (device, nullable = identity): int32 [n,4] = flags (bit0 flip x, bit1 flip y), ty, tx, 0;
 * tone (device, nullable = none): fp32 [n,2] = gain, offset.  Canvas pixel (y,x) of image i, fp32 arithmetic without contraction:
 *   ys = y - ty, xs = x - tx, inside = 0 <= ys < H && 0 <= xs < W;  flags&2: ys = H-1-ys;  flags&1: xs = W-1-xs   (flip over the full H, W)
 *   r = inside ? img[i,c,ys,xs] : 0;  x01 = r | float(r)/65535 | float(r)/255;
 *   tone && (gain,offset) != (1,0): x01 = min(max(gain*x01 + offset, 0), 1);  v = scale16 ? (x01*65535 - 32767.5)/32767.5 : x01;  out = bf16(v)
 * Any ty / tx / flags is safe (the inside test guards the only read); no host copy of the tables is needed.  With fp32 input and NULL
 * tables the result is mmg_patchify's, bit for bit.  Additive entry point: mmg_abi_version() stays 5. */
int mmg_patchify_aug(const void* img, int src_kind, void* out, int n, int Cin, int H, int W, int P, int Kp, int scale16,
                     const int* geom, const float* tone, mmg_stream_t stream);

/* torch.optim.AdamW step over a flat fp32 buffer (mmgclip/experiments/ClassifierExperiment.py:74,118);
 * p_bf16 (nullable) receives the refreshed bf16 working copy.  step counts from 1. */
int mmg_adamw_step(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, float grad_scale, mmg_stream_t stream);

/* ---- gradient clipping by global norm + non-finite-step guard (csrc/grad_clip.hip) ------------------------------
 * The reference goes from loss.backward() straight to optimizer.step() (mmgclip/experiments/ClassifierExperiment.py:115-118);
 * these sit between the two, where a user would call torch.nn.utils.clip_grad_norm_.  Additive entry points: they came
 * without an ABI version step (mmg_abi_version() stays 5).  No host read-back, no atomics, no memset; bit-reproducible. */

/* Number of per-workgroup partial sums mmg_grad_sumsq writes for n elements: clamp(ceil(n / 8192), 1, 2048); 0 for n <= 0.
 * A function of n alone (never of the device), so the same gradient gives the same bits everywhere. */
int mmg_grad_sumsq_partials(long long n);
/* partials[w] = sum of g[i]^2 over the elements workgroup w reads, squared and accumulated in fp64 (n_partials must equal
 * mmg_grad_sumsq_partials(n)).  Any n >= 1; g needs 4-byte alignment only (views, 0-d tensors).  Beside
 * ClassifierExperiment.py:115-118 (additive). */
int mmg_grad_sumsq(const float* g, long long n, double* partials, int n_partials, mmg_stream_t stream);
/* The n partials of every gradient buffer of the step (back to back), summed in a fixed order in fp64:
 *   out[0] = total_norm (fp32),  out[1] = min(1, max_norm / (total_norm + 1e-6)) (torch.nn.utils.clip_grad_norm_; exactly 1 for
 *   max_norm <= 0 or +inf = no clipping),  out[2] = 1 if total_norm is finite as fp32, else 0;
 * when it is not finite and skipped != NULL: *skipped += 1.  Beside ClassifierExperiment.py:115-118 (additive). */
int mmg_grad_clip_finalize(const double* partials, int n, float max_norm, float* out, int* skipped, mmg_stream_t stream);
/* mmg_adamw_step with the gradient scale and the go/no-go taken from the device: clip = the `out` above, g is multiplied by
 * clip[1]; skipped != NULL: when clip[2] == 0 nothing is written (p, m, v, p_bf16 keep their bits), else the bias corrections
 * use t = step - *skipped, so a skipped step does not advance Adam's clock; skipped == NULL: always steps, t = step.
 * Beside ClassifierExperiment.py:115-118 (additive). */
int mmg_adamw_step_guarded(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, float lr, float beta1,
                           float beta2, float eps, float weight_decay, int step, const float* clip, const int* skipped,
                           mmg_stream_t stream);
/* mmg_adamw_step / mmg_adamw_step_guarded over an arena whose parameters sit in several torch param groups, in one launch
 * (csrc/adamw_groups.hip).  The reference hands torch.optim.AdamW ONE group (ClassifierExperiment.py:74); param groups are torch's own
 * means for no-decay sets and layer-wise learning rates (additive, mmg_abi_version() stays 5).  chunk_group (device, n / 64 bytes):
 * the group of elements [64 c, 64 c + 64) - params.ParamArena starts every parameter on a 64-element boundary; a chunk whose byte
 * is >= n_groups is left untouched.  group_lr / group_wd are HOST arrays of n_groups floats, read during the call and passed to the
 * kernel by value: they may change at every step.  n a multiple of 64, 1 <= n_groups <= 128, p / g / m / v 16-byte aligned.
 * clip == NULL (then skipped must be NULL): mmg_adamw_step's arithmetic with grad_scale 1; clip given: mmg_adamw_step_guarded's. */
int mmg_adamw_step_groups(float* p, const float* g, float* m, float* v, long long n, const unsigned char* chunk_group, int n_groups,
                          const float* group_lr, const float* group_wd, float beta1, float beta2, float eps, int step,
                          const float* clip, const int* skipped, mmg_stream_t stream);

/* ConvNeXt layer scale (out = x + gamma * (G W2^T + b2)): converts the unscaled weight-gradient GEMM results
 * dW2raw [C,K], db2raw [C] into dgamma, dW2, db2 (all ACCUMULATED).  torchvision CNBlock.layer_scale. */
int mmg_layerscale_finalize(const float* W2, const float* b2, const float* gamma, const float* dW2raw,
                            const float* db2raw, float* dW2, float* db2, float* dgamma, int C, int K,
                            mmg_stream_t stream);
/* dst += relayout(src): mode 0 = [R,(kh,kw,ci)] -> [R,CI,KH,KW] (patchify-conv weight gradients),
 * mode 1 = [49,R] -> [R,49] (depthwise taps). */
int mmg_grad_relayout(const float* src, float* dst, int mode, int R, int CI, int KH, int KW, int ld_src,
                      mmg_stream_t stream);

/* ---- stochastic depth, "row" mode (csrc/stochastic_depth.hip) ------------------------------------------------
 * torchvision CNBlock.stochastic_depth = StochasticDepth(p, "row") of the ConvNeXt behind mmgclip/networks/encoder.py:53 (the reference runs
 * it frozen, where it is the identity).  A block's dropped samples are not computed at all: the images of a micro-batch are reordered so that
 * the kept ones are a prefix, and the block's kernels run on that prefix.  Activations are bf16 [n, rows, C]; C % 8 == 0 and 16-byte aligned
 * pointers (16-byte accesses, 64-bit offsets); every element touched is written once, no atomics.  Additive entry points: mmg_abi_version()
 * stays 5.
 * mmg_image_swap: IN PLACE, exchange image pairs[p][0] with image pairs[p][1] for p < k.  pairs: device int32 [k][2]; pairs_host: the same
 *   table in host memory - it is what is validated before the launch (every index inside 0 .. n-1, no image in two pairs).  k = 0: no launch.
 * mmg_image_copy: dst[first .. first+count) = src[first .. first+count) (whole images; src != dst).  count = 0: no launch. */
int mmg_image_swap(void* x, const int* pairs, const int* pairs_host, int k, int n, long long rows, int C, mmg_stream_t stream);
int mmg_image_copy(const void* src, void* dst, int first, int count, int n, long long rows, int C, mmg_stream_t stream);
/* dst += alpha * src (fp32 [n]).  With stochastic depth the layer scale the kernels see is gamma / (1 - p): mmg_layerscale_finalize then
 * yields d/d(that product) into a temporary, and this folds it into the gradient of gamma with alpha = 1 / (1 - p). */
int mmg_scaled_add_f32(float* dst, const float* src, float alpha, long long n, mmg_stream_t stream);

/* Inverted dropout on fp32 (projection heads: mmgclip/networks/projection.py:50,59,91,98); keep = uint8 mask. */
int mmg_dropout_fwd(const float* x, float* y, void* keep, long long n, float p, long long seed, mmg_stream_t stream);
int mmg_dropout_bwd(const float* dy, const void* keep, float* dx, long long n, float p, mmg_stream_t stream);

/* ---- depthwise 7x7 convolution, NHWC bf16 (ConvNeXt CNBlock) ------------------------------------------------ */

/* y = dwconv7x7(x; w, bias) (+ add), padding 3; x,y,add bf16 [n,H,W,C]; w fp32 tap-major [49][C]
 * (w[kh*7+kw][c] = weight[c,0,kh,kw]); flip != 0 reverses the taps (data gradient when x := dy).
 * C % 32 == 0.  Replaces CNBlock.block[0] of torchvision ConvNeXt (mmgclip/networks/encoder.py:53). */
int mmg_dwconv7_nhwc(const void* x, const float* w, const float* bias, const void* add, void* y, int n, int H, int W,
                     int C, int flip, mmg_stream_t stream);
/* The same contract on the matrix cores (ABI 5, csrc/dwconv7_mfma.hip): per channel and kernel row the 1-D convolution along x is a product with a
 * banded Toeplitz matrix (v_mfma_f32_16x16x32_bf16, taps rounded to bf16, fp32 accumulation); the NHWC <-> channel-plane layout changes run on the
 * LDS transposed reads.  With `add` the fp32 sum is rounded to bf16 once, as in mmg_dwconv7_nhwc (it was rounded twice - convolution, then + add - until tests/test_dwconv_gpu.py held both kernels to one bar).  (Rounds 1 - 2 had an earlier kernel of this name,
 * at parity with the VALU one and removed in ABI 4.) */
int mmg_dwconv7_nhwc_mfma(const void* x, const float* w, const float* bias, const void* add, void* y, int n, int H, int W,
                          int C, int flip, mmg_stream_t stream);
/* dw[49][C] += sum x(shifted) * dy ; dbias[C] += sum dy  (fp32, accumulated; dbias nullable) */
int mmg_dwconv7_wgrad(const void* x, const void* dy, float* dw, float* dbias, int n, int H, int W, int C,
                      mmg_stream_t stream);
/* What a depthwise 7x7 entry point WOULD launch, without launching: the plan its host layer makes (csrc/dwconv_plan.h; the three entry points
 * validate, make one plan and launch the kernel it names) as text - the exact mmg_last_kernel() spelling, then
 * " grid=(x,y,z) block=T lds=B nt=0|1 tile=HxW items=N" (B = dynamic LDS bytes, nt = the output is stored past L2: 256 MiB and more, never the
 * weight gradient; tile = pixels per tile; N = n x tiles, the (image, tile) pairs of one 32-channel slab) and, for op 1, " add=0|1 by_image=0|1"
 * (the ADD instantiation, which the kernel's name does not spell; by_image: n >= 8, an image's tiles stay with one XCD group).
 * op: 0 mmg_dwconv7_nhwc, 1 mmg_dwconv7_nhwc_mfma, 2 mmg_dwconv7_wgrad; flip, add (ops 0, 1): as the entry point's flip, and whether its add
 * operand is given; cus (read by op 1 only): CU count the plan is made for, 0 = the current device's.  MMG_DWCONV_ROWS2 / MMG_DWCONV_TH /
 * MMG_DWG_TH / MMG_DWG_ALIGN / MMG_DWM_WAVES are honoured as by a launch.  A shape the entry point would reject gives "" and sets
 * mmg_last_error() to that entry point's message.  The string belongs to the calling thread and is valid until its next call; no GPU is
 * needed unless op == 1 and cus == 0.  No reference counterpart (diagnostics; tests/test_dwconv_plan_cpu.py pins kernel selection and launch
 * geometry with it).  Additive entry point: mmg_abi_version() stays 5. */
const char* mmg_dwconv7_plan(int op, int n, int H, int W, int C, int flip, int add, int cus);

/* ---- fused ConvNeXt block MLP (C in {96,128,192,256,384,512}) ---------------------------------------------------------- */

/* What mmg_cnblock_mlp_fwd (op 0), mmg_cnblock_mlp_bwd (op 1) or mmg_cnblock_bwdw (op 2) would launch for M rows of width C, as text:
 * the kernel instantiation as mmg_last_kernel() spells it (op 2: both launches, "cnblock_bwdw_kernel<..> + <..>"), then
 * " grid=G block=T lds=B nt=0|1 tiles=N" (workgroups, threads - op 2: "block=(T1,T2)" -, dynamic LDS bytes, nt = the 4C-wide outputs are
 * stored past L2, N = tiles walked).  save (op 0 only): the forward saves hpre and the row statistics; ln (op 1 only): ln_dw / ln_db are
 * given; cus: CU count the plan is made for, 0 = the current device's.  MMG_MLP_FWD_RES / MMG_MLP_NT_STORE / MMG_BWDW_VAR / MMG_BWDW_HTO /
 * MMG_BWDW_W12 are honoured as by a launch.  A shape the entry point would reject gives "" and sets mmg_last_error() to that entry point's
 * message.  The string belongs to the calling thread and is valid until its next call; no GPU is needed when cus != 0.  No reference
 * counterpart (diagnostics; tests/test_cnblock_plan_cpu.py pins kernel selection with it).  Additive entry point: mmg_abi_version() stays 5. */
const char* mmg_cnblock_plan(int op, long long M, int C, int save, int ln, int cus);

/* Number of bf16 elements of the packed weight image (8C^2 forward / backward=2, 12C^2 backward=1); 0 when C is unsupported. */
long long mmg_cnblock_packed_elems(int C, int backward);
/* Pack W1 fp32 [4C,C], W2 fp32 [C,4C] (torchvision CNBlock.block[3] / block[5]) into the per-chunk LDS images the fused
 * kernels stream (layout: csrc/cnblock_mlp.hip).  backward = 1 builds [W1 | gamma*W2^T | W1^T], backward = 2 builds [gamma*W2^T | W1^T]; both need gamma [C]. */
int mmg_cnblock_pack_weights(const float* w1, const float* w2, const float* gamma, void* packed, int C, int backward,
                             mmg_stream_t stream);
/* y = residual + gamma * ( GELU( LayerNorm(xd; ln_w, ln_b, eps) W1^T + b1 ) W2^T + b2 ), rows of [M,C] bf16.
 * Replaces CNBlock.block[2..5] + layer_scale + residual of torchvision ConvNeXt (mmgclip/networks/encoder.py:53) in one
 * launch: the 4C-wide hidden row stays in registers.  hpre (bf16 [M,4C], pre-GELU) and mean/rstd (fp32 [M]) are optional (all three or none)
 * outputs for a backward that does not recompute them; xln (bf16 [M,C], the LayerNorm output = operand of that backward's
 * weight-gradient GEMM; optional, only next to hpre) saves it a LayerNorm pass; gact (bf16 [M,4C], GELU(hidden) as the second GEMM
 * consumed it; optional, only next to hpre) is the operand of that backward's dW2 GEMM, which lets its data-gradient GEMM run
 * epilogue 5 (GELU' only) instead of 2.  hpre_kind = 1 (ABI 5; needs hpre and gact): `hpre` receives GELU'(hidden) instead of the hidden -
 * that data-gradient GEMM then runs epilogue 7, a multiply.  (ABI 2: xln added; ABI 4: gact added.) */
int mmg_cnblock_mlp_fwd(const void* xd, const float* ln_w, const float* ln_b, float eps, const void* packed,
                        const float* b1, const float* b2, const float* gamma, const void* residual, void* y, void* hpre,
                        void* xln, void* gact, float* mean, float* rstd, int hpre_kind, long long M, int C, mmg_stream_t stream);

/* Data path of the CNBlock MLP backward in one launch.  mmg_cnblock_mlp_bwd_supported(C): 1 (C in {96,128,192}) = the
 * hidden row h = LN(xd) W1^T + b1 is recomputed from the saved depthwise output, packed_bwd = pack(..., backward=1), hpre must
 * be NULL and the forward saves nothing 4C-wide; 2 (C = 384) = h is read back from the forward's hpre, packed_bwd =
 * pack(..., backward=2); 0 = unsupported.  Writes g = GELU(h), dh = (dy gamma W2) * GELU'(h) (bf16 [M,4C], operands of the
 * weight-gradient GEMMs dW2 = dy^T g, dW1 = dh^T xln), xln = LN(xd) and dxln = dh W1 (bf16 [M,C]) and the LN statistics for
 * mmg_layernorm_bwd.  With ln_dw / ln_db (fp32 [C], accumulated) the LayerNorm backward is fused into the epilogue: dxln then
 * receives d loss / d xd and no mmg_layernorm_bwd launch is needed.
 * (New capability: the reference never trains the image tower, mmgclip/networks/encoder.py:53.) */
int mmg_cnblock_mlp_bwd_supported(int C);
int mmg_cnblock_mlp_bwd(const void* dy, const void* xd, const float* ln_w, const float* ln_b, float eps,
                        const void* packed_bwd, const float* b1, const void* hpre, void* dh, void* g, void* xln,
                        void* dxln, float* mean, float* rstd, float* ln_dw, float* ln_db, long long M, int C,
                        mmg_stream_t stream);

/* CNBlock MLP backward with the weight gradients accumulated ON CHIP (round 3; C = 96, M a multiple of 64): nothing 4C-wide
 * reaches HBM.  Two launches (csrc/cnblock_bwdw.hip): (1) h = LN(xd) W1^T + b1, g = GELU(h), dW2raw += dy^T g, db2raw += colsum(dy);
 * (2) h again, dh = (dy gamma W2) * GELU'(h), dW1 += dh^T LN(xd), db1 += colsum(dh), d LN-out = dh W1, LayerNorm backward:
 * dd = d loss / d xd (bf16 [M,C]), ln_dw / ln_db += LayerNorm weight / bias gradients.  All fp32 outputs are ACCUMULATED (atomics);
 * dW2raw / db2raw are the un-scaled gradients mmg_layerscale_finalize expects (the same contract as dy^T g of the GEMM path).
 * `packed` / `b1f` come from mmg_cnblock_bwdw_pack (bf16 mmg_cnblock_bwdw_packed_elems(C) elements; fp32 [4C]): the W1 LDS image,
 * the LayerNorm-folded W1 and layer-scale-folded W2^T as per-wave MFMA fragments, and b1' = b1 + W1 ln_b.
 * Replaces autograd of CNBlock.block[2..5] + layer_scale (torchvision ConvNeXt; the reference runs it frozen, encoder.py:53). */
int mmg_cnblock_bwdw_supported(int C);
long long mmg_cnblock_bwdw_packed_elems(int C);
int mmg_cnblock_bwdw_pack(const float* w1, const float* w2, const float* ln_w, const float* ln_b, const float* layer_scale,
                          const float* b1, void* packed, float* b1f, int C, mmg_stream_t stream);
int mmg_cnblock_bwdw(const void* dy, const void* xd, const float* ln_w, const float* ln_b, float eps, const void* packed,
                     const float* b1f, void* dd, float* dW1, float* db1, float* dW2raw, float* db2raw, float* ln_dw,
                     float* ln_db, long long M, int C, mmg_stream_t stream);

/* ConvNeXt stem (features[0]: Conv2d(Cin, C, 4, 4) as a GEMM over mmg_patchify's rows, then LayerNorm2d) in two launches
 * (csrc/stem.hip); the [M,C] tensors s0 = p0 w^T + bias and ds0 that the three-launch path (mmg_gemm_nt, mmg_layernorm_fwd;
 * mmg_layernorm_bwd, mmg_gemm_tn_acc) stores between its kernels never reach memory.  mmg_stem_supported(C, kp): C in {96, 128} and
 * kp in {32, 64}; any M >= 1 (rows are addressed with 64-bit offsets: no 4 GiB range to split a launch at).
 * p0: bf16 [M,kp]; w: bf16 [C,kp] (the working copy of the conv weight, zero-padded to kp); bias, ln_w, ln_b: fp32 [C].
 * mmg_stem_fwd: x (bf16 [M,C]) = LN(bf16(p0 w^T + bias)) - the product accumulates in fp32 and is rounded to bf16 BEFORE the
 * LayerNorm, as the stored s0 was; mean / rstd (fp32 [M]): the row statistics of that rounded s0, both NULL for a pass that saves nothing.
 * mmg_stem_bwd: recomputes s0 (rounded to bf16) from p0, forms xhat from the saved statistics, runs the LayerNorm backward in registers,
 * rounds ds0 to bf16 as the stored tensor was, and ACCUMULATES (fp32 atomics, once per workgroup) dW [C,kp] += ds0^T p0,
 * db [C] += colsum(ds0), ln_dw [C] += sum dx xhat, ln_db [C] += colsum(dx).  Nothing [M,C]-wide is written.
 * Replaces autograd of torchvision ConvNeXt features[0] (the reference runs the tower frozen, mmgclip/networks/encoder.py:53).
 * Additive entry points: mmg_abi_version() stays 5. */
int mmg_stem_supported(int C, int kp);
int mmg_stem_fwd(const void* p0, const void* w, const float* bias, const float* ln_w, const float* ln_b, float eps, void* x,
                 float* mean, float* rstd, long long M, int C, int kp, mmg_stream_t stream);
int mmg_stem_bwd(const void* dx, const void* p0, const void* w, const float* bias, const float* ln_w, const float* mean,
                 const float* rstd, float* dW, float* db, float* ln_dw, float* ln_db, long long M, int C, int kp,
                 mmg_stream_t stream);

/* Data-gradient GEMM with the LayerNorm backward in its epilogue (csrc/gemm_lnbwd.hip): the two launches mmg_gemm_nt_bf16 (dln = A B^T,
 * bf16) + mmg_layernorm_bwd (dln, x -> dx) in one, with their roundings; dln is never stored.  A: bf16 [M,K], B: bf16 [N,K];
 * dln = bf16(A B^T) (fp32 accumulation); per pixel (C consecutive columns of a row): xhat = (x - mean) rstd, g = dln gamma,
 * dx = bf16(rstd (g - mean_C(g) - xhat mean_C(g xhat))); dgamma [C] += sum dln xhat, dbeta [C] += sum dln (fp32 atomics, once per
 * workgroup; both may be NULL).  patch = 0: N == C, GEMM row r is LayerNorm row r.  patch = 1: N == 4 C, row r = (n, ph, pw) and its
 * segment s are pixel (n, 2 ph + s / 2, 2 pw + s % 2) of an H x W map; x, dx (bf16 [pixels, C]), mean, rstd (fp32 [pixels]) by pixel.
 * mmg_gemm_nt_lnbwd_supported: N % 384 == 0, K % 64 == 0, K >= 64, C in {96, 192, 384}, N == C (patch 0) or 4 C (patch 1), and for
 * patch 1 even H and W (odd maps keep the two launches).  The launch also needs M >= 1 and, for patch 1, M a multiple of (H/2)(W/2).
 * Everything is validated before any HIP call; an unsupported shape returns non-zero and launches nothing.
 * Additive entry points: mmg_abi_version() stays 5. */
int mmg_gemm_nt_lnbwd_supported(int N, int K, int C, int patch, int H, int W);
int mmg_gemm_nt_lnbwd(const void* A, int lda, const void* B, int ldb, int M, int N, int K, const void* x, int ldx,
                      const float* mean, const float* rstd, const float* gamma, void* dx, int lddx, float* dgamma, float* dbeta,
                      int C, int patch, int H, int W, mmg_stream_t stream);

/* ---- AveragedMedicalCLIPLoss helpers (reference mmgclip/loss/losses.py:98-216) ------------------------------------------------ */

/* `_assign_labels` (losses.py:148-162) on the device: walking i = 0..n-1, an unlabelled text opens the next cluster and every
 * still unlabelled j > i with sim[i][j] >= threshold joins it.  sim fp32 [n,n] (ld); labels int64 [n]; counts int32 [n]
 * (members per cluster, first *k_out entries valid); k_out int32 device scalar = number of clusters.  n <= 16384. */
int mmg_greedy_threshold_labels(const float* sim, int ld, int n, float threshold, long long* labels, int* counts, int* k_out,
                                mmg_stream_t stream);

/* `_average_logits` (losses.py:164-186): out[i,c] = mean_{j: labels[j]==c} logits[i,j]  (logits fp32 [n,N], out fp32 [n,k]),
 * and its backward dlogits[i,j] = dout[i,labels[j]] / counts[labels[j]]. */
int mmg_cluster_mean_cols_fwd(const float* logits, int ld, int n, int N, const long long* labels, const int* counts, int k,
                              float* out, int ldo, mmg_stream_t stream);
int mmg_cluster_mean_cols_bwd(const float* dout, int ldo, int n, int N, const long long* labels, const int* counts,
                              float* dlogits, int ld, mmg_stream_t stream);

/* The same loss from the (gathered) L2-normalised embeddings, no [n,N] logits (mmgclip/loss/losses.py:164-216).  By linearity the
 * column-averaged logits are s <I_i, Tbar_c> with Tbar_c the mean text embedding of cluster c, so both cross-entropies are
 * "rows of X [n_loc,D] against Y [M,D] with an int64 label per row" (image side: Y = Tbar, M = k; text side: Y = I, M = N).
 * D % 32 == 0, 32 <= D <= 1024; n_loc, M > 0.
 *
 * mmg_clip_labelled_rows_fwd:  lse[r] = logsumexp_m( s <X_r,Y_m> ),  pos[r] = s <X_r, Y_{row_label[r]}>  (losses.py:164-216;
 *   a label outside [0,M) matches no column: pos = 0). */
int mmg_clip_labelled_rows_fwd(const float* X, const float* Y, const float* scale, const long long* row_label, int n_loc, int M,
                               int D, float* lse, float* pos, mmg_stream_t stream);
/* Gradient products dX[r,:] (+)= s * sum_m g[r,m] Y[m,:]  (accumulate != 0 adds into dX), z = s <X_r,Y_m>, gout a device scalar
 * (NULL = 1), coef = 1/(2 N_global); autograd of losses.py:164-216 through the two logit products:
 *   _row:  g[r,m] = coef gout ( exp(z - lse_row[r]) - [m == row_label[r]] );  dscale += sum g[r,m] <X_r,Y_m>  (dscale may be NULL)
 *   _col:  g[r,m] = coef gout w[r] ( exp(z - lse_col[m]) - [col_label[m] == key[r]] ),  lse_col / col_label: [M] (the transposed
 *          problem's row log-sum-exps and labels),  key[r] = row_key ? row_key[r] : key_off + r,
 *          w[r] = counts ? 1 / counts[key[r]] : 1  (counts int32 [n_counts]; needs row_key).  No dscale: each softmax element is
 *          counted once, by its _row product. */
int mmg_clip_labelled_rows_bwd_row(const float* X, const float* Y, const float* scale, const float* lse_row,
                                   const long long* row_label, const float* gout, float coef, int n_loc, int M, int D,
                                   int accumulate, float* dX, float* dscale, mmg_stream_t stream);
int mmg_clip_labelled_rows_bwd_col(const float* X, const float* Y, const float* scale, const float* lse_col,
                                   const long long* col_label, const long long* row_key, int key_off, const int* counts,
                                   int n_counts, const float* gout, float coef, int n_loc, int M, int D, int accumulate,
                                   float* dX, mmg_stream_t stream);
/* Cluster centroids (the column average of losses.py:164-186 moved onto the embeddings): out[c,:] = mean_{j: labels[j]==c} T[j,:],
 * T fp32 [N,D], out fp32 [k,D].  Members are added in ascending j by one wave per cluster, no float atomics: the same bits in give
 * the same bits out on every rank and in every run.  N <= 16384, 1 <= k <= N. */
int mmg_cluster_centroids(const float* T, const long long* labels, int N, int D, int k, float* out, mmg_stream_t stream);

/* Sigmoid pairwise loss (SigLIP, Zhai et al. 2023; the reference has no such loss) of the n_loc local rows X against the N gathered
 * rows Y (both L2-normalised, [.,D] fp32; D % 32 == 0, 32 <= D <= 1024), without an [n_loc,N] matrix in HBM:
 *   z_ij = s <X_i,Y_j> + b   (s = *scale, the exponentiated scale; b = *bias; device scalars),   y_ij = +1 for a positive pair, else -1
 *   positive: col_label == NULL ? j == diag_off + i : col_label[j] == row_key[i]   (int64 [N] / [n_loc]; both or neither)
 * _fwd: row_loss[i] = sum_j softplus(-y_ij z_ij), softplus(u) = max(u,0) + log1p(exp(-|u|)).  One fp32 per row, written (not
 *       accumulated) by its single owner in a fixed order, no atomics: bit-identical from run to run.
 * _bwd: g_ij = coef * gout * (-y_ij) * sigmoid(-y_ij z_ij)   (gout: device scalar, NULL = 1);   dX[i,:] = s * sum_j g_ij Y[j,:] (written);
 *       dscale += sum_ij g_ij <X_i,Y_j> (w.r.t. the exponentiated scale, as mmg_clip_rows_bwd_fused);  dbias += sum_ij g_ij;
 *       either may be NULL; one float atomic per 32 rows each.
 * Rows and columns the 32 x 32 tiles pad add exactly nothing.  Additive entry points: mmg_abi_version() stays 5. */
int mmg_sigmoid_rows_fwd(const float* X, const float* Y, const float* scale, const float* bias, const long long* row_key,
                         const long long* col_label, int n_loc, int N, int D, int diag_off, float* row_loss, mmg_stream_t stream);
int mmg_sigmoid_rows_bwd(const float* X, const float* Y, const float* scale, const float* bias, const long long* row_key,
                         const long long* col_label, const float* gout, float coef, int n_loc, int N, int D, int diag_off,
                         float* dX, float* dscale, float* dbias, mmg_stream_t stream);

/* Retrieval ranks (validation; the reference has no such metric): where the best positive of each of the n_loc local queries X stands
 * among the negatives of the N gallery rows Y ([.,D] fp32; D % 32 == 0, 32 <= D <= 1024), without an [n_loc,N] matrix in HBM and
 * without a sort.  s_ij = <X_i,Y_j>: no scale or bias (a positive scale does not change a rank).
 *   positive: col_label == NULL ? j == diag_off + i : col_label[j] == row_key[i]   (int64 [N] / [n_loc]; both or neither; on the
 *             diagonal 0 <= diag_off and diag_off + n_loc <= N)
 *   n_pos[i] = number of positives;  best[i] = max of s_ij over them, -inf when there is none;
 *   n_gt[i] / n_eq[i] = number of NEGATIVE j with s_ij > best[i] / s_ij == best[i]   (a positive never counts; with no positive
 *             every column is a negative above -inf).  The host takes rank_i = 1 + n_gt[i] + n_eq[i]: ties count against the model.
 * One launch, two sweeps over Y (the threshold, then the counts), both through the same MFMA chain, so `==` compares equal bits.
 * Integer counts, one owner per row, a fixed tree, no atomics: bit-identical from run to run and however the queries are split over
 * launches.  Rows and columns the 32 x 32 tiles pad are never counted or written.  FINITE inputs are assumed: a NaN score compares
 * false both ways and is not defined here.  Additive entry point: mmg_abi_version() stays 5. */
int mmg_retrieval_rows_rank(const float* X, const float* Y, const long long* row_key, const long long* col_label, int n_loc, int N,
                            int D, int diag_off, float* best, int* n_pos, int* n_gt, int* n_eq, mmg_stream_t stream);

/* Nearest-neighbour search: the k best gallery columns of every local query, without an [n_loc,N] matrix (csrc/topk_head.hip; the
 * reference has no search, its PromptClassifier scores a handful of prompts densely, mmgclip/networks/mmgclip_model.py:168-257).
 * X [n_loc,D], Y [N,D] fp32; scores fp32 / indices int32 [n_loc,k] row-major; D % 32 == 0, 32 <= D <= 1024, 1 <= k <= 32.
 *   s_ij = <X_i,Y_j> (no scale, no bias; the bits of mmg_retrieval_rows_rank's scores);  column j has the global index J = j_base + j
 *   excluded: exclude 0 none (row_key, col_label NULL) | 1 J == diag_off + i (both NULL, diag_off >= 0; a diagonal outside this chunk
 *             excludes nothing) | 2 col_label[j] == row_key[i] (int64 [N] / [n_loc], both given)
 *   row i receives its k best admissible columns under the TOTAL order (score descending, then J ascending): scores as fp32, indices
 *   as J; slots beyond the number of admissible columns hold -inf / -1 (k > N is legal).
 *   accumulate != 0: the buffers hold a valid list (sorted by that order, padded with -inf / -1) from launches over OTHER columns;
 *   the result is the top-k of the union.  accumulate == 0: every owned element is written, nothing beyond row n_loc is.
 * The order is total, so the result is unique: bit-identical however the gallery is cut into launches, whichever rows share a launch
 * and from run to run.  No atomics.  FINITE inputs are assumed; NaN is not defined.  j_base >= 0 and j_base + N fits int32.
 * mmg_topk_rows_supported: 1 / 0, whether the staged rows (32 (D+4) 4 bytes) and the lists (4 x 32 x k x 8 bytes) fit the 160 KB of LDS:
 * every D <= 992 with k <= 32, D = 1024 with k <= 31.  mmg_topk_rows_lds_bytes: the launch's dynamic LDS, 0 when unsupported.  Neither
 * makes a HIP call; everything is validated before any HIP call.  Additive entry points: mmg_abi_version() stays 5. */
int mmg_topk_rows_supported(int D, int k);
int mmg_topk_rows_lds_bytes(int D, int k);
int mmg_topk_rows(const float* X, const float* Y, int n_loc, int N, int D, int k, int exclude, const long long* row_key,
                  const long long* col_label, int diag_off, int j_base, int accumulate, float* scores, int* indices,
                  mmg_stream_t stream);

/* Linear probe on frozen embeddings: the un-normalised loss, weight gradient and bias gradient of a multinomial logistic regression
 * out of ONE read of X (csrc/probe_head.hip; the reference scores a shipped classifier head instead, mmgclip/evaluator.py
 * evaluate_cnn / clf_conf_matrix).  X [n,D], W [C,D], b [C] fp32 contiguous (X, W 16-byte aligned); labels int64 [n]; class_weight
 * fp32 [C] or NULL (weight 1); D % 32 == 0, 32 <= D <= 1024, 2 <= C <= 32, n >= 1.
 *   z_ic = <X_i,W_c> + b_c;  w_i = class_weight[labels[i]];  a row whose label is outside [0,C) is ignored (the host admits -1 only)
 *   L = sum_i w_i (logsumexp_c z_ic - z_{i,labels[i]});  dW[c][d] = sum_i w_i (p_ic - [c == labels[i]]) X[i][d];  db[c] likewise
 *   out: fp64 [C (D+1) + 1] = dW | db as [C][D+1] row-major (column D is db), then L.  The host divides by sum_i w_i and adds L2.
 * n_groups persistent workgroups (0 = one per CU; never more than ceil(n/32)), workgroup g takes the 32-row blocks g, g + n_groups, ..
 * and writes partials[g] = { fp64 loss, fp32 [C][D+1] }, 8 + 4 C (D+1) bytes rounded up to 8; a second launch sums the partials in
 * index order in fp64 into out.  partials and out 8-byte aligned; partials holds mmg_probe_rows_partials_bytes(n, D, C, n_groups)
 * bytes (0 for arguments mmg_probe_rows rejects; n_groups <= 4096), every byte the second launch reads is written by the first.
 * No atomics, one owner per element: bit-identical from run to run; a different n_groups regroups the fp32 sums.  p is e / sum by a
 * true division (W = 0 with C a power of two gives exactly 1/C); padded classes and rows are selected to zero.  FINITE inputs.
 * mmg_probe_rows_supported: 1 / 0 for (D, C), no HIP call.  mmg_probe_rows_partials_bytes with n_groups = 0 asks the CURRENT device
 * for its CU count (HIP calls; 256 without a device), so it must be queried with the device current that will launch; with
 * n_groups > 0 it makes no HIP call.  Everything is validated before any HIP call.  Additive entry points:
 * mmg_abi_version() stays 5. */
int mmg_probe_rows_supported(int D, int C);
long long mmg_probe_rows_partials_bytes(int n, int D, int C, int n_groups);
int mmg_probe_rows(const float* X, const float* W, const float* b, const long long* labels, const float* class_weight, int n, int D,
                   int C, int n_groups, void* partials, double* out, mmg_stream_t stream);

/* Zero-shot AUROC with bootstrap replicates as exact integer pair counts (validation / evaluation; csrc/auroc_head.hip).
 *   U2[b] = sum_{i<P} sum_{j<Nn} w_pos[b][i] * w_neg[b][j] * g(s_pos[i], s_neg[j]),  g = 2 [s+ > s-] + [s+ == s-],
 *   AUROC_b = U2[b] / (2 * sum_i w_pos[b][i] * sum_j w_neg[b][j])   (the host divides; weights all 1 = the point estimate).
 * s_pos [P], s_neg [Nn] fp32, finite normal numbers or zero (NaN and denormals are not defined); w_pos [B][ldw_pos], w_neg [B][ldw_neg]
 * int8 in 0..127, replicate-major; ldw_* a multiple of 16 and at least P / Nn (so at least the width padded to 16); the columns
 * Nn .. ldw_neg-1 of w_neg hold 0; s_neg and w_neg 16-byte aligned.  partial: int64 [ceil(P/32)][B], every element written; the host
 * sums the row blocks in int64.  v_mfma_i32_32x32x32_i8, int32 accumulators: the caller guarantees 2 * max_b sum_j w_neg[b][j] < 2^31.
 * One owner per (row block, replicate), a fixed integer tree, no atomics, no memset: bit-identical from run to run and however the
 * positives are split over launches.  Rows beyond P and columns beyond Nn add exactly nothing. */
int mmg_auroc_pairs(const float* s_pos, const float* s_neg, const signed char* w_pos, int ldw_pos, const signed char* w_neg,
                    int ldw_neg, int P, int Nn, int B, long long* partial, mmg_stream_t stream);

/* Bootstrap multiplicities: w[b - b0][t] (int8, row stride ldw, a multiple of 16 and >= n; w 16-byte aligned) = how many of replicate
 * b's n draws landed on sample t, for b = b0 .. b0+B-1 (B <= 65535); columns n .. ldw-1 are written as 0.  Draw t' of replicate b is
 *   idx = (mmg_drop_bits(t', mmg_drop_key_bh(mmg_drop_key(seed, 0x200), b)) * n) >> 32      (the hash of csrc/dropout.h)
 * - a pure function of (seed, b, t'); the multiply-high's bias is below n / 2^32 per value.  Integer LDS counters, no scratch.  A count
 * above 127 does not wrap: it is written as -128 and the host raises on any negative weight. */
int mmg_bootstrap_weights(unsigned long long seed, int n, int b0, int B, signed char* w, int ldw, mmg_stream_t stream);

/* ---- fp8 (OCP e4m3) forward GEMM path: BASELINE config C5 "ConvNeXt-base fp8 MFMA path" ---------------------------------
 * The reference has no reduced-precision path (its towers run torch fp32, mmgclip/networks/encoder.py:53,156); these replace
 * the same nn.Linear forwards of torchvision's CNBlock as mmg_gemm_nt_bf16 does, on v_mfma_f32_16x16x128_f8f6f4 (twice the
 * bf16 MFMA rate, half the operand bytes).  Backward stays bf16 (saved pre-activations and bf16 weight copies). */

/* C[M,N] = epilogue( alpha * (alpha_dev ? *alpha_dev : 1) * A[M,K] B[N,K]^T + bias ): A, B e4m3 bytes row-major (K contiguous,
 * lda / ldb in bytes, multiples of 16), fp32 accumulate.  Epilogue as mmg_gemm_nt_bf16 with epi in {0 none, 1 GELU, 3 ReLU, 6 GELU + GELU' side output};
 * out_kind: 0 bf16 | 1 fp32 | 2 e4m3 bytes (saturating at +-448; ldc in elements of that type).  K % 128 == 0, N % 8 == 0.
 * alpha_dev: device scalar, e.g. scales[1] of mmg_quantize_e4m3_f32 (so weight scales never visit the host). */
int mmg_gemm_nt_fp8(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                    const float* bias, const float* colscale, const void* residual, int ldr, void* aux_out, int ldao,
                    int epi, int out_kind, float alpha, const float* alpha_dev, mmg_stream_t stream);

/* ---- fp8 backward of the ConvNeXt blocks (ABI 5; BASELINE config C5 "ConvNeXt-base fp8 MFMA path"; the reference itself has no fp8) ---------- */

/* src bf16 [n] -> dst OCP e5m2 bytes [n] with the per-tensor power-of-two scale 2^floor(log2(16384 / max|src|)) computed on the device
 * (amax fp32 [1] is scratch); scales fp32 [2] = (scale, 1 / scale).  n % 8 == 0.  The gradient entering a CNBlock backward
 * (torchvision CNBlock behind mmgclip/networks/encoder.py:53). */
int mmg_quantize_e5m2_bf16(const void* src, long long n, float* amax, void* dst, float* scales, mmg_stream_t stream);
/* The same in ONE pass ("delayed scaling"): scale = 2^floor(log2(4096 / *amax_prev)) from the absmax this tensor had at its previous quantisation
 * (1 when that is 0), and the tensor's own absmax is left in amax_next (fp32 [1]) for the next call. */
int mmg_quantize_e5m2_bf16_delayed(const void* src, long long n, const float* amax_prev, float* amax_next, void* dst, float* scales,
                                   mmg_stream_t stream);
/* The delayed cast of a gradient MATRIX src bf16 [M, C] (contiguous) and colsum[c] += sum_m src[m][c] (fp32 [C]) in one pass over src: the bias gradient
 * of a CNBlock's second Linear is taken from the bf16 gradient, not from its cast.  C = 16 x a divisor of 256 (256, 512, 1024 ... of ConvNeXt-B). */
int mmg_quantize_e5m2_colsum_bf16(const void* src, int M, int C, const float* amax_prev, float* amax_next, void* dst, float* scales,
                                  float* colsum, mmg_stream_t stream);
/* C[M,N] = epilogue( alpha * alpha_dev * alpha_dev2 * A[M,K] B[N,K]^T ): A = e5m2 (a_e5m2 != 0) or e4m3 bytes, B e4m3 bytes, fp32 accumulate on the
 * K = 128 MFMA; epi 0 none | 5 multiply by GELU'(aux_in) | 7 multiply by aux_in (aux_in bf16 [M,N]); C bf16 / fp32 / e5m2 bytes (out_kind 0 / 1 / 3).
 * The two data-gradient GEMMs of a CNBlock (dh = (dy (gamma W2)) * GELU'(h) handed on in 8 bits, d LN-out = dh W1).  K % 128 == 0. */
int mmg_gemm_nt_fp8_bwd(const void* A, int lda, int a_e5m2, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                        const void* aux_in, int ldai, int epi, int out_kind, float alpha, const float* alpha_dev,
                        const float* alpha_dev2, mmg_stream_t stream);
/* C[N1,N2] (fp32) += alpha * alpha_dev * A[M,N1]^T B[M,N2]: A e5m2 (a_e5m2 != 0) or e4m3 bytes, B e4m3 bytes, both row-major with the reduction index
 * slow (transposed 8-bit fragment reads, ds_read_b64_tr_b8); colsum_a [N1] (optional) += alpha * alpha_dev * column sums of A.  N1, N2, lda, ldb
 * multiples of 16.  The two weight-gradient GEMMs of a CNBlock on the 8-bit operands its forward / data-gradient GEMMs already hold. */
int mmg_gemm_tn_fp8(const void* A, int lda, int a_e5m2, const void* B, int ldb, float* C, int ldc, int M, int N1, int N2,
                    float alpha, const float* alpha_dev, float* colsum_a, mmg_stream_t stream);

/* amax[0] = max(amax[0], max |src[i]|) (caller zeroes amax);  then  dst = e4m3(src * scale) with the power-of-two
 * scale = 2^floor(log2(448 / amax)) (1 when amax is null / 0), scales[0] = scale, scales[1] = 1 / scale.  n % 4 == 0. */
int mmg_absmax_f32(const float* src, long long n, float* amax, mmg_stream_t stream);
int mmg_quantize_e4m3_f32(const float* src, long long n, const float* amax, void* dst, float* scales, mmg_stream_t stream);

/* mmg_layernorm_fwd whose output row is written as e4m3 bytes (unscaled, saturating; ldy in bytes, multiple of 8). */
int mmg_layernorm_fwd_fp8(const void* x, int ldx, const float* gamma, const float* beta, float eps, void* y8, int ldy,
                          float* mean, float* rstd, int M, int C, mmg_stream_t stream);

/* ---- ResNet-50 tower pieces (reference ResNet50Encoder, mmgclip/networks/encoder.py:57-119: torchvision resnet50 minus fc,
 * everything frozen except layer4).  NHWC bf16; convolutions = im2col + mmg_gemm_nt_bf16 (1x1: no im2col at all). ------------ */

/* col[n*Ho*Wo, Kp] (bf16) from x[n,H,W,C]: column (kh*KW + kw)*C + c, zeros outside the image and in the K padding; C % 8 == 0. */
int mmg_im2col_nhwc(const void* x, void* col, int n, int H, int W, int C, int KH, int KW, int stride, int pad, int Kp,
                    mmg_stream_t stream);
/* dx[n,H,W,C] = adjoint of mmg_im2col_nhwc applied to dcol (data gradient of a k x k convolution); gather, no atomics. */
int mmg_col2im_nhwc(const void* dcol, void* dx, int n, int H, int W, int C, int KH, int KW, int stride, int pad, int Kp,
                    mmg_stream_t stream);
/* nn.MaxPool2d(3, stride 2, padding 1) forward (encoder.py:107). */
int mmg_maxpool3x3s2_nhwc(const void* x, void* y, int n, int H, int W, int C, mmg_stream_t stream);
/* nn.BatchNorm2d on rows [M = n*H*W, C]: column sums of x and x^2 (fp64 [C] each, accumulated; zero them first).  fp64 because the
 * variance is sumsq / M - mean^2: fp32 sums lose mean^2 / var of their precision, fp64 ones keep rstd and running_var at fp32. ... */
int mmg_bn_stats_f64(const void* x, int M, int C, double* sum, double* sumsq, mmg_stream_t stream);
/* ... -> mean / rstd and the fused affine (scale, shift), each formed in fp64 and rounded to fp32 once.  train != 0: batch statistics
 * (biased variance) and torch's running-statistics update with `momentum` (unbiased variance; running_mean / running_var a nullable
 * pair); train == 0: the running statistics are used and sum / sumsq may be NULL. */
int mmg_bn_finalize_f64(const double* sum, const double* sumsq, int M, int C, const float* gamma, const float* beta, float eps,
                        float momentum, float* running_mean, float* running_var, int train, float* mean, float* rstd,
                        float* scale, float* shift, mmg_stream_t stream);
/* y = x * scale[c] + shift[c] (+ residual) (ReLU when relu != 0): bn + the bottleneck's shortcut add + ReLU in one pass. */
int mmg_bn_apply(const void* x, const float* scale, const float* shift, const void* residual, void* y, int M, int C, int relu,
                 mmg_stream_t stream);
/* Training-mode backward of y = relu?(bn(x) (+ residual)): g = dy masked by `out` > 0 (the layer's own output; NULL = no ReLU).
 * reduce: sum_g[c] += g, sum_gx[c] += g * xhat (= d beta, d gamma).  apply: dx = gamma rstd (g - sum_g/M - xhat sum_gx/M);
 * dres (nullable) = g, the gradient of the residual branch; dgamma / dbeta (nullable pair, fp32 [C]) += sum_gx / sum_g. */
int mmg_bn_bwd_reduce(const void* dy, const void* x, const void* out, const float* mean, const float* rstd, int M, int C,
                      float* sum_g, float* sum_gx, mmg_stream_t stream);
int mmg_bn_bwd_apply(const void* dy, const void* x, const void* out, const float* mean, const float* rstd, const float* gamma,
                     const float* sum_g, const float* sum_gx, int M, int C, void* dx, void* dres, float* dgamma, float* dbeta,
                     mmg_stream_t stream);

/* ---- BERT attention / embeddings / pooling -------------------------------------------------------------------- */

/* ctx[B*S,Hd] = per-head softmax(Q K^T * scale + key mask) V with qkv = [B*S, q|k|v] bf16 (head h at columns h*64
 * of each third); mask int64 [B,S] (1 attend / 0 pad, nullable); lse fp32 [B,heads,S] (nullable) for the backward.
 * head_dim 64, S <= 512.  The mask may be any 0/1 pattern (not only a right-padded prefix); the result for a sequence whose
 * mask row is all zero is unspecified.  Replaces HF BertSelfAttention (mmgclip/networks/encoder.py:156). */
int mmg_attention_fwd(const void* qkv, int ld, const long long* mask, void* ctx, int ldc, float* lse, int B, int S,
                      int heads, int Hd, float scale, mmg_stream_t stream);
/* dqkv (same layout as qkv) from dctx; recomputes probabilities from lse.  S <= 256. */
int mmg_attention_bwd(const void* qkv, int ld, const long long* mask, const void* ctx, int ldc, const float* lse,
                      const void* dctx, int lddc, void* dqkv, int lddq, int B, int S, int heads, int Hd, float scale,
                      mmg_stream_t stream);

/* Flash-style tiled attention for sequences of any length (ViT-B/16 on 1024x1024: S = 4097; BERT training at S > 256):
 * same layout and semantics as mmg_attention_fwd/bwd, K/V (or Q/dO) streamed through LDS in 64-row tiles, online
 * softmax, no S x S tensor.  delta_ws: caller-provided fp32 [B*heads*S] scratch. */
int mmg_attention_long_fwd(const void* qkv, int ld, const long long* mask, void* ctx, int ldc, float* lse, int B, int S,
                           int heads, int Hd, float scale, mmg_stream_t stream);
int mmg_attention_long_bwd(const void* qkv, int ld, const long long* mask, const void* ctx, int ldc, const float* lse,
                           const void* dctx, int lddc, void* dqkv, int lddq, float* delta_ws, int B, int S, int heads,
                           int Hd, float scale, mmg_stream_t stream);

/* The same attention on the packed ("unpadded") layout: sequence b occupies rows cu_seqlens[b] .. cu_seqlens[b+1] of qkv / ctx /
 * dctx / dqkv (int32 [B+1], device), every token attended, lengths in [1, S_max]; lse is [B, heads, S_max].  The reference pads
 * every prompt to max_length (mmgclip/dataset/dataset.py:347) and reads only the [SEP] row (mmgclip_model.py:110-111): the
 * text tower runs on the valid tokens only and scatters its last hidden state back into the padded layout. */
int mmg_attention_varlen_fwd(const void* qkv, int ld, const int* cu_seqlens, void* ctx, int ldc, float* lse, int B, int S_max,
                             int heads, int Hd, float scale, mmg_stream_t stream);
int mmg_attention_varlen_bwd(const void* qkv, int ld, const int* cu_seqlens, const void* ctx, int ldc, const float* lse,
                             const void* dctx, int lddc, void* dqkv, int lddq, int B, int S_max, int heads, int Hd,
                             float scale, mmg_stream_t stream);

/* Training-mode dropout of the text tower.  The reference runs HF BertModel under model.train()
 * (mmgclip/experiments/ClassifierExperiment.py:97 -> mmgclip/networks/encoder.py:156) with hidden_dropout_prob =
 * attention_probs_dropout_prob = 0.1 (notebooks/bert_experimental.ipynb:609-624).  Masks are counter-based (csrc/dropout.h;
 * restated in oracle/dropout_oracle.py): element `index` of dropout site `site` is kept, and scaled by 1/(1-p), iff
 * fmix32(index * 0x9E3779B1 + key(seed, site)) >= floor(p * 2^32) - the backward regenerates the mask from (p, seed, site).
 *   mmg_attention_dropout_fwd/_bwd: the whole-sequence attention above (S <= 512 forward, <= 256 backward; _long_bwd beyond) with the
 *     probabilities dropped before P V; cu_seqlens != NULL selects the packed layout (then `mask` is unused), else the padded one.
 *     index = (((first_sequence + b) * heads + h) * 512 + query) * 512 + key  (first_sequence: position of this call's
 *     sequence 0 in the whole batch, so that micro-batches of one batch draw disjoint masks).
 *   mmg_dropout_f32 : x fp32 [M,C] <- dropout(x) in place, optional bf16 copy xb.    index = token * C + column, token = rows[m]
 *   mmg_dropout_bf16: out bf16 [M,C] = dropout(in)  (the same mask on a gradient).    (rows NULL: token = m).
 * p in [0,1); p = 0 is the identity. */
int mmg_attention_dropout_fwd(const void* qkv, int ld, const long long* mask, const int* cu_seqlens, void* ctx, int ldc,
                              float* lse, int B, int S, int heads, int Hd, float scale, float p, unsigned long long seed,
                              unsigned site, int first_sequence, mmg_stream_t stream);
int mmg_attention_dropout_bwd(const void* qkv, int ld, const long long* mask, const int* cu_seqlens, const void* ctx, int ldc,
                              const float* lse, const void* dctx, int lddc, void* dqkv, int lddq, int B, int S, int heads,
                              int Hd, float scale, float p, unsigned long long seed, unsigned site, int first_sequence,
                              mmg_stream_t stream);
/* the same backward for 256 < S <= 512 (padded layout only): tiled dQ / dK,dV kernels; delta_ws = fp32 [B * heads * S] workspace */
int mmg_attention_dropout_long_bwd(const void* qkv, int ld, const long long* mask, const void* ctx, int ldc, const float* lse,
                                   const void* dctx, int lddc, void* dqkv, int lddq, float* delta_ws, int B, int S, int heads,
                                   int Hd, float scale, float p, unsigned long long seed, unsigned site, int first_sequence,
                                   mmg_stream_t stream);
int mmg_dropout_f32(float* x, int ldx, void* xb, int ldb, const long long* rows, long long M, int C, float p,
                    unsigned long long seed, unsigned site, mmg_stream_t stream);
int mmg_dropout_bf16(const void* in, int ldi, void* out, int ldo, const long long* rows, long long M, int C, float p,
                     unsigned long long seed, unsigned site, mmg_stream_t stream);

/* out[m,:] = word[ids[m]] + pos[m % S] + type[type_ids[m]] (bf16 tables [V|P|T, H]); HF BertEmbeddings before its
 * LayerNorm (mmgclip/networks/encoder.py:156). */
int mmg_bert_embed_fwd(const long long* ids, const long long* type_ids, const void* word, const void* pos,
                       const void* type, void* out, int M, int S, int H, int V, int T, mmg_stream_t stream);
/* table gradients (fp32, accumulated) from g = d out [B*S,H] bf16 */
int mmg_bert_embed_bwd(const void* g, const long long* ids, const long long* type_ids, float* dword, float* dpos,
                       float* dtype, int B, int S, int H, int V, int T, mmg_stream_t stream);

/* EOS pooling: out[b,:] (fp32) = hidden[b, sum(mask[b])-1, :]; idx_out (int32 [B], nullable) keeps the index.
 * Replaces mmgclip/networks/mmgclip_model.py:110-111. */
int mmg_eos_pool_fwd(const void* hidden, const long long* mask, float* out, int* idx_out, int B, int S, int H,
                     mmg_stream_t stream);
/* the same from an fp32 hidden state [B*S, H] (the text tower's fp32 residual stream) */
int mmg_eos_pool_fwd_f32(const float* hidden, const long long* mask, float* out, int* idx_out, int B, int S, int H,
                         mmg_stream_t stream);
int mmg_eos_pool_bwd(const float* dout, const int* idx, void* dhidden, int B, int S, int H, mmg_stream_t stream);

/* ViT token assembly (torchvision VisionTransformer: class token + patch tokens + encoder.pos_embedding):
 * out[b,0,:] = cls + pos[0]; out[b,1+p,:] = tok[b*Np+p,:] + pos[1+p]; S = Np + 1; all bf16. */
int mmg_vit_assemble_fwd(const void* tok, const void* cls, const void* pos, void* out, int B, int S, int H,
                         mmg_stream_t stream);
/* dtok (bf16) = g rows 1..; dpos[S,H] += sum_b g; dcls[H] += sum_b g[b,0,:]  (fp32, accumulated) */
int mmg_vit_assemble_bwd(const void* g, void* dtok, float* dpos, float* dcls, int B, int S, int H, mmg_stream_t stream);
/* out[b,:] (fp32) = hidden[b*S + idx[b], :] — pooling at explicit token indices (class token: idx = 0);
 * its backward is mmg_eos_pool_bwd. */
int mmg_gather_rows_fwd(const void* hidden, const int* idx, float* out, int B, int S, int H, mmg_stream_t stream);

/* ---- patch dropout for the ViT tower (csrc/patch_dropout.hip) ---------------------------------------------------
 * FLIP (Li et al. 2023) / open_clip's `patch_dropout`: under train() an image keeps K of its P patches plus the class token and the
 * encoder runs on 1 + K tokens.  No reference counterpart (its image encoders are ConvNeXt-T / ResNet-50, mmgclip/networks/encoder.py:15,57).
 * Every argument is validated before any HIP call; no atomics, one writer per element: bit-reproducible.  K in 1 .. P everywhere.
 * Additive entry points: mmg_abi_version() stays 5.
 * mmg_patch_keep_indices: the draw of csrc/dropout.h under site 0x50447270,
 *     bits_p = mmg_drop_bits(p, mmg_drop_key_bh(mmg_drop_key(seed, site), (unsigned) sample_ids[b])),   sample_ids NULL: sample id b;
 *   image b keeps the K patches with the smallest bits_p (a bijection of p: no ties).  keep int32 [B,K]: their indices, ascending;
 *   slot int32 [B,P]: the position of patch p among the kept ones of image b, or -1.  sample_ids: device int64 [B] or NULL.
 *   One workgroup per image, the keys in LDS: P <= 16384. */
int mmg_patch_keep_indices(unsigned long long seed, const long long* sample_ids, int B, int P, int K, int* keep, int* slot,
                           mmg_stream_t stream);
/* The foreground prior: the same draw made aware of the image, in two launches (additive: mmg_abi_version() stays 5).
 * mmg_patch_foreground: counts int32 [n, (H/patch)*(W/patch)], counts[i,p] = the foreground elements among the Cin*patch*patch canvas
 *   elements of patch p, under mmg_patchify_aug's geometry to the letter: src_kind 0 = fp32, 1 = uint16, 2 = uint8; geom (device, nullable =
 *   identity) int32 [n,4] = flags, ty, tx, 0; the same inside test, flips over the full H, W and fill; remainder rows / columns beyond
 *   floor(H/patch)*patch, floor(W/patch)*patch ignored.  A canvas element is foreground iff inside && x01 > threshold, x01 = r |
 *   float(r)/65535 | float(r)/255 in fp32 (IEEE division), BEFORE any tone: what is tissue does not depend on the brightness jitter.  A fill
 *   pixel and a NaN are background.  threshold in [0, 1).  Every pixel is read once, coalesced along x for any W and row alignment; integer
 *   counts, no global atomics, one writer per output.
 * mmg_patch_keep_indices_prior: patch p of image b is foreground iff counts[b,p] >= min_pixels (>= 1), and the image keeps the K patches
 *   smallest under (0 if foreground else 1, bits_p), bits_p as in mmg_patch_keep_indices: every foreground patch before any background
 *   patch, the hash inside each class.  nfg >= K: a hash-uniform K-subset of the foreground; nfg < K: all of it plus the K - nfg background
 *   patches of smallest bits; a row of one class (nfg 0 or NP) equals mmg_patch_keep_indices' row bit for bit.  keep, slot: as there;
 *   n_foreground (nullable) int32 [B] = nfg.  One workgroup per image, keys and class flags in LDS: NP <= 16384. */
int mmg_patch_foreground(const void* img, int src_kind, int n, int Cin, int H, int W, int patch, const int* geom, float threshold,
                         int* counts, mmg_stream_t stream);
int mmg_patch_keep_indices_prior(unsigned long long seed, const long long* sample_ids, const int* counts, int min_pixels, int B, int NP,
                                 int K, int* keep, int* slot, int* n_foreground, mmg_stream_t stream);
/* out bf16 [B*K,Kp] = the rows b*P + keep[b,j] of p0 bf16 [B*P, Kp] (row stride ld elements); Kp % 8 == 0, ld % 8 == 0, 16-byte aligned. */
int mmg_gather_patch_rows(const void* p0, long long ld, const int* keep, void* out, int B, int P, int K, int Kp, mmg_stream_t stream);
/* mmg_vit_assemble_fwd on the kept tokens, positions as before the drop: out bf16 [B, 1+K, H];
 * out[b,0,:] = cls + pos[0]; out[b,1+j,:] = tok[b*K+j,:] + pos[1+keep[b,j],:]; pos is the full table [1+P, H].  H % 8 == 0. */
int mmg_vit_assemble_keep_fwd(const void* tok, const void* cls, const void* pos, const int* keep, void* out, int B, int P, int K,
                              int H, mmg_stream_t stream);
/* g bf16 [B, 1+K, H] -> dtok bf16 [B*K, H] = g rows 1..; dpos fp32 [1+P, H]: dpos[1+p] += the sum, in ascending b, of g[b, 1+slot[b,p]] over
 * the images that kept p (a row that nobody kept is not touched); dpos[0] and dcls[H] += sum_b g[b,0,:]: the bits of mmg_vit_assemble_bwd
 * on the full gradient that is zero at the dropped rows. */
int mmg_vit_assemble_keep_bwd(const void* g, const int* slot, void* dtok, float* dpos, float* dcls, int B, int P, int K, int H,
                              mmg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGCLIP_HIP_H */
