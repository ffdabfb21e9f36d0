// Contrastive head for mmg-clip on gfx950: L2-normalise, logits = s * X Y^T, symmetric
// cross-entropy and their backward, in fp32 on the f32-input MFMA (v_mfma_f32_32x32x2_f32).
//
// Reference arithmetic being replaced (citations into /root/reference):
//   mmgclip/networks/mmgclip_model.py:128-136  (e / ||e||, exp(logit_scale), two [n,n] matmuls)
//   mmgclip/loss/losses.py:36-44               (CLIPLoss: (CE(Li,arange)+CE(Lt,arange))/2)
//   mmgclip/loss/losses.py:74-91               (MMGCLIPLoss: same CE on recomputed logits + t2t term)
//
// Design: the [n_local, N] logit tile never has to reach HBM.  A workgroup owns 32 local rows i,
// keeps their embeddings in LDS and streams 32-column tiles of the gathered matrix Y.  The MFMA is
// issued "swapped" (A = Y tile, B = X tile) so each lane holds ONE row i (its column of the
// accumulator) and 16 columns j in registers: the row max / sum of the softmax are register-local
// and need a single lane^32 shuffle at the end.  In the backward the accumulator registers are fed
// back as the A operand of the second product (dX = G Y) with no lane movement.  Both kernels are
// written once in clip_tile.h for all three heads; this file holds CLIP's label source and pair rules.
#include "clip_tile.h"

// ---------------------------------------------------------------------------------------------
// L2 normalise rows (no epsilon, as the reference): y = x / ||x||_2
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         float* __restrict__ norm, int rows, int D) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= rows) return;
    const float* xr = x + (size_t)r * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) { float v = xr[c]; s += v * v; }
    s = wave_sum(s);
    const float nrm = sqrtf(s);
    float* yr = y + (size_t)r * D;
    for (int c = lane; c < D; c += 64) yr[c] = xr[c] / nrm;
    if (lane == 0) norm[r] = nrm;
}

// dx = (dy - y * <y, dy>) / ||x||
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ y, const float* __restrict__ norm,
                                                         const float* __restrict__ dy, float* __restrict__ dx,
                                                         int rows, int D) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= rows) return;
    const float* yr = y + (size_t)r * D;
    const float* gr = dy + (size_t)r * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += yr[c] * gr[c];
    s = wave_sum(s);
    const float inv = 1.0f / norm[r];
    float* dr = dx + (size_t)r * D;
    for (int c = lane; c < D; c += 64) dr[c] = (gr[c] - yr[c] * s) * inv;
}

// ---------------------------------------------------------------------------------------------
// Cross-entropy over materialised logits (CLIPLoss / AveragedMedicalCLIPLoss operands):
// one wave per row; loss_sum += weight * (lse - z[label]).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ce_rows_fwd_kernel(const float* __restrict__ logits, int ld,
                                                          const long long* __restrict__ labels, int rows, int C,
                                                          float weight, float* __restrict__ lse,
                                                          float* __restrict__ loss_sum) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= rows) return;
    const float* zr = logits + (size_t)r * ld;
    float m = NEG_BIG;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, zr[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += __expf(zr[c] - m);
    s = wave_sum(s);
    if (lane == 0) {
        const float l = m + __logf(s);
        lse[r] = l;
        const long long lab = labels ? labels[r] : (long long)r;
        atomicAdd(loss_sum, weight * (l - zr[lab]));
    }
}

// dlogits[r,c] = gout * weight * (exp(z - lse[r]) - [c == label])
__global__ __launch_bounds__(256) void ce_rows_bwd_kernel(const float* __restrict__ logits, int ld,
                                                          const long long* __restrict__ labels,
                                                          const float* __restrict__ lse, const float* __restrict__ gout,
                                                          float weight, int rows, int C, float* __restrict__ dlogits,
                                                          int ldd) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= rows) return;
    const float g = weight * (gout ? *gout : 1.0f);
    const float l = lse[r];
    const long long lab = labels ? labels[r] : (long long)r;
    const float* zr = logits + (size_t)r * ld;
    float* dr = dlogits + (size_t)r * ldd;
    for (int c = lane; c < C; c += 64) dr[c] = g * (__expf(zr[c] - l) - (c == lab ? 1.0f : 0.0f));
}

// loss = coef * (sum(lse_a - pos_a) + sum(lse_b - pos_b)) accumulated into *loss (one block)
__global__ __launch_bounds__(256) void clip_loss_reduce_kernel(const float* __restrict__ lse_a,
                                                               const float* __restrict__ pos_a,
                                                               const float* __restrict__ lse_b,
                                                               const float* __restrict__ pos_b, int n, float coef,
                                                               float* __restrict__ loss) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        s += lse_a[i] - pos_a[i];
        if (lse_b) s += lse_b[i] - pos_b[i];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss, coef * (red[0] + red[1] + red[2] + red[3]));
}

// =============================================================================================
// C ABI
// =============================================================================================
MMG_API int mmg_l2norm_fwd(const float* x, float* y, float* norm, int rows, int D, hipStream_t stream) {
    MMG_CHECK_ARG(x && y && norm && rows > 0 && D > 0, "mmg_l2norm_fwd: bad argument");
    hipLaunchKernelGGL(l2norm_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, x, y, norm, rows, D);
    MMG_LAUNCH_CHECK("mmg_l2norm_fwd");
    return 0;
}

MMG_API int mmg_l2norm_bwd(const float* y, const float* norm, const float* dy, float* dx, int rows, int D,
                           hipStream_t stream) {
    MMG_CHECK_ARG(y && norm && dy && dx && rows > 0 && D > 0, "mmg_l2norm_bwd: bad argument");
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, y, norm, dy, dx, rows, D);
    MMG_LAUNCH_CHECK("mmg_l2norm_bwd");
    return 0;
}

// label(i) = diag_off + i: the positive of local row i in the gathered matrix
struct DiagLabel {
    using arg = int;
    using type = int;
    static constexpr const char* NOTE = "rows_lse_fwd_kernel<DiagLabel, %s>";
    static __device__ __forceinline__ int of(int diag_off, int ig, int) { return diag_off + ig; }
};

MMG_API int mmg_clip_rows_fwd(const float* X, const float* Y, const float* scale, int n_loc, int N, int D,
                              int diag_off, float* lse, float* pos, float* logits, int ldl, hipStream_t stream) {
    if (rows_check_dims("mmg_clip_rows_fwd", n_loc, N, D)) return 1;
    MMG_CHECK_ARG(X && Y && scale && lse && pos, "mmg_clip_rows_fwd: null pointer");
    MMG_CHECK_ARG(!logits || ldl >= N, "mmg_clip_rows_fwd: ldl=%d < N=%d", ldl, N);
    if (logits) launch_rows_lse_fwd<DiagLabel, true>(X, Y, scale, diag_off, n_loc, N, D, lse, pos, logits, ldl, stream);
    else launch_rows_lse_fwd<DiagLabel, false>(X, Y, scale, diag_off, n_loc, N, D, lse, pos, nullptr, 0, stream);
    MMG_LAUNCH_CHECK("mmg_clip_rows_fwd");
    return 0;
}

// Pair rules of rows_bwd_kernel (clip_tile.h), with z_ij = s <X_i, Y_j>:
//   fused : g_ij = coef * gout * (exp(z_ij - lse_row[i]) + exp(z_ij - lse_col[j]) - 2 [j == diag_off+i])
//           (the gradient of the symmetric CE w.r.t. z_ij when lse_row / lse_col are the row and the
//            column log-sum-exps of the GLOBAL logit matrix; coef = dloss / (2 N_global))
//   dense : g_ij = Ga[i*lda + j] + Gb[j*ldb + i]   (upstream gradients of materialised logits and of
//            their transposed twin, either may be null)
struct ClipFusedPair {
    static constexpr bool DSCALE = true, DBIAS = false, ACCUMULATE = false;
    static constexpr const char* NOTE = "rows_bwd_kernel<ClipFusedPair, %d>";
    const float *lse_row, *lse_col, *gout;
    float coef;
    int diag_off;
    struct Row {
        float lr, c_up;
        int lab;
    };
    __device__ __forceinline__ Row row(int ig, int n_loc) const {
        return {ig < n_loc ? lse_row[ig] : 0.f, coef * (gout ? *gout : 1.0f), diag_off + ig};
    }
    __device__ __forceinline__ float g(const Row& w, float dot, float scale, int j) const {
        const float z = dot * scale;
        float g = __expf(z - w.lr) + __expf(z - lse_col[j]);
        if (j == w.lab) g -= 2.0f;
        return g * w.c_up;
    }
};

struct ClipDensePair {
    static constexpr bool DSCALE = true, DBIAS = false, ACCUMULATE = false;
    static constexpr const char* NOTE = "rows_bwd_kernel<ClipDensePair, %d>";
    const float* Ga;
    int lda;
    const float* Gb;
    int ldb;
    struct Row {
        int ig;
    };
    __device__ __forceinline__ Row row(int ig, int) const { return {ig}; }
    __device__ __forceinline__ float g(const Row& w, float, float, int j) const {
        float g = 0.f;
        if (Ga) g += Ga[(size_t)w.ig * lda + j];
        if (Gb) g += Gb[(size_t)j * ldb + w.ig];
        return g;
    }
};

// Fused symmetric-CE gradient of the rows.  dscale (may be null) is ACCUMULATED.
MMG_API int mmg_clip_rows_bwd_fused(const float* X, const float* Y, const float* scale, const float* lse_row,
                                    const float* lse_col, const float* gout, float coef, int n_loc, int N, int D,
                                    int diag_off, float* dX, float* dscale, hipStream_t stream) {
    if (rows_check_dims("mmg_clip_rows_bwd_fused", n_loc, N, D)) return 1;
    MMG_CHECK_ARG(X && Y && scale && lse_row && lse_col && dX, "mmg_clip_rows_bwd_fused: null pointer");
    launch_rows_bwd(X, Y, scale, ClipFusedPair{lse_row, lse_col, gout, coef, diag_off}, n_loc, N, D, 0, dX, dscale, nullptr, stream);
    MMG_LAUNCH_CHECK("mmg_clip_rows_bwd_fused");
    return 0;
}

// Backward of materialised logits: dX = s * (Ga + Gb^T) Y ; dscale += <Ga + Gb^T, X Y^T>.
MMG_API int mmg_clip_rows_bwd_dense(const float* X, const float* Y, const float* scale, const float* Ga, int lda,
                                    const float* Gb, int ldb, int n_loc, int N, int D, float* dX, float* dscale,
                                    hipStream_t stream) {
    if (rows_check_dims("mmg_clip_rows_bwd_dense", n_loc, N, D)) return 1;
    MMG_CHECK_ARG(X && Y && scale && dX && (Ga || Gb), "mmg_clip_rows_bwd_dense: null pointer");
    MMG_CHECK_ARG((!Ga || lda >= N) && (!Gb || ldb >= n_loc), "mmg_clip_rows_bwd_dense: bad leading dimension");
    launch_rows_bwd(X, Y, scale, ClipDensePair{Ga, lda, Gb, ldb}, n_loc, N, D, 0, dX, dscale, nullptr, stream);
    MMG_LAUNCH_CHECK("mmg_clip_rows_bwd_dense");
    return 0;
}

MMG_API int mmg_ce_rows_fwd(const float* logits, int ld, const long long* labels, int rows, int C, float weight,
                            float* lse, float* loss_sum, hipStream_t stream) {
    MMG_CHECK_ARG(logits && lse && loss_sum && rows > 0 && C > 0 && ld >= C, "mmg_ce_rows_fwd: bad argument");
    hipLaunchKernelGGL(ce_rows_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, logits, ld, labels, rows, C,
                       weight, lse, loss_sum);
    MMG_LAUNCH_CHECK("mmg_ce_rows_fwd");
    return 0;
}

MMG_API int mmg_ce_rows_bwd(const float* logits, int ld, const long long* labels, const float* lse, const float* gout,
                            float weight, int rows, int C, float* dlogits, int ldd, hipStream_t stream) {
    MMG_CHECK_ARG(logits && lse && dlogits && rows > 0 && C > 0 && ld >= C && ldd >= C, "mmg_ce_rows_bwd: bad argument");
    hipLaunchKernelGGL(ce_rows_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, logits, ld, labels, lse, gout,
                       weight, rows, C, dlogits, ldd);
    MMG_LAUNCH_CHECK("mmg_ce_rows_bwd");
    return 0;
}

MMG_API int mmg_clip_loss_reduce(const float* lse_a, const float* pos_a, const float* lse_b, const float* pos_b, int n,
                                 float coef, float* loss, hipStream_t stream) {
    MMG_CHECK_ARG(lse_a && pos_a && loss && n > 0 && (!lse_b || pos_b), "mmg_clip_loss_reduce: bad argument");
    hipLaunchKernelGGL(clip_loss_reduce_kernel, dim3(1), dim3(256), 0, stream, lse_a, pos_a, lse_b, pos_b, n, coef, loss);
    MMG_LAUNCH_CHECK("mmg_clip_loss_reduce");
    return 0;
}
