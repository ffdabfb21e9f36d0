// Linear probe on frozen embeddings: loss, softmax and the WEIGHT gradient of a multinomial logistic regression out of ONE read of X.
// The reference scores a shipped classifier head instead (Evaluator.evaluate_cnn, clf_conf_matrix); this is an additive head on the
// tile skeleton of clip_tile.h: a classifier with C <= 32 classes is exactly one 32-row tile of "Y", and the second product runs in the
// direction the skeleton's backward does not have (rows_bwd_kernel gives dX = G Y, this gives dW = G^T X).
//
//   z_ic    = <X_i, W_c> + b_c                       (c < C; a padded class enters neither the maximum, the sum nor the gradient)
//   w_i     = class_weight[y_i] (1 without a table); a row with y_i outside [0,C) is IGNORED (w_i = 0, skipped; the host admits -1 only)
//   L       = sum_i w_i (logsumexp_c z_ic - z_{i,y_i})
//   dW[c,d] = sum_i w_i (p_ic - [c == y_i]) X[i,d],   db[c] = sum_i w_i (p_ic - [c == y_i]),   p_ic = exp(z_ic - m_i) / sum_c exp(z_ic - m_i)
// The sums are UN-normalised: the host divides by S = sum_i w_i and adds the L2 term.
//
// Data flow.  A grid of G persistent workgroups; workgroup g takes the 32-row blocks g, g+G, ..  Per block:
//   1. stage_x: the 32 rows into LDS (rows beyond n are clamped duplicates).
//   2. Z^T tile: the K range is cut into four quarters, wave w runs zt_tile over [w D/4, (w+1) D/4) against W (lane il holds W row
//      min(il, C-1)) and parks its partial tile in LDS.
//   3. wave 0 alone: the four partials summed in one fixed tree, the bias, the masked softmax of a row across the two lane halves
//      (a lane holds one row and 16 classes), p = e / sum (a true division: W = 0 with C a power of two gives exactly 1/C), and the
//      G tile parked in LDS row-major, g_ic SELECTED to zero for a padded class, a row beyond n and an ignored row; the row's loss.
//   4. second product dW^T tile += G^T X on v_mfma_f32_32x32x2_f32, K = the row index, both operands from LDS; wave w owns the d tiles
//      w, w+4, ..; the accumulators STAY IN REGISTERS across all of the workgroup's blocks.  32 threads of wave 3 add the block's
//      column sums of G to db in row order, one thread adds the 32 row losses in row order into an fp64 sum.
// At the end workgroup g writes partials[g] = { fp64 loss, fp32 [C][D+1] (column D = db) }.  probe_finalize_kernel sums the G partials
// in index order in fp64.  No atomics, one owner per element: two launches on the same inputs give the same bits.  FINITE inputs.
#include <math.h>

#include "clip_tile.h"

#define PROBE_MAX_C 32
#define PROBE_MAX_GROUPS 4096
#define PROBE_LDS_LIMIT 163840          // 160 KB of LDS per workgroup on gfx950
#define PROBE_TILE (32 * 33)            // one parked 32 x 32 tile, pitch 33

// bytes of one workgroup's partial: the fp64 loss, then [C][D+1] fp32, rounded up to 8
static inline size_t probe_partial_stride(int D, int C) { return (8 + (size_t)C * (D + 1) * 4 + 7) / 8 * 8; }
static inline size_t probe_lds_bytes(int D) { return rows_lds_bytes(D, 4 * PROBE_TILE + PROBE_TILE + 32); }

template <int NDT>
__global__ __launch_bounds__(CLIP_THREADS) void probe_rows_kernel(
    const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias, const long long* __restrict__ labels,
    const float* __restrict__ class_weight, int n, int D, int C, int G, unsigned char* __restrict__ partials, size_t stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int xld = D + 4;
    float* Xs = smem;                        // [32 rows][xld]
    float* Zs = smem + CLIP_ROWS * xld;      // [4 waves][32 classes][33]: the K quarters of the Z^T tile
    float* Gs = Zs + 4 * PROBE_TILE;         // [32 rows][33]: the G tile, row-major
    float* Ls = Gs + PROBE_TILE;             // [32]: the rows' losses
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int il = lane & 31, h = lane >> 5;
    const int nblocks = (n + CLIP_ROWS - 1) / CLIP_ROWS;
    const int ndtiles = D / 32;
    const int kq = D / 4;                    // a multiple of 8: one wave's share of K

    f32x16 dacc[NDT];
#pragma unroll
    for (int t = 0; t < NDT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[t][r] = 0.f;
    float db = 0.f;                          // wave 3, lane c < 32
    double loss = 0.0;                       // wave 3, lane 32

    const float* wrow = W + (size_t)min(il, C - 1) * D + wave * kq;
    float bc[16];                            // wave 0: the bias of this lane's 16 classes
#pragma unroll
    for (int r = 0; r < 16; ++r) bc[r] = bias[min(acc_row(r, h), C - 1)];

    for (int blk = blockIdx.x; blk < nblocks; blk += G) {
        const int i0 = blk * CLIP_ROWS;
        __syncthreads();                     // the previous block's second product is done with Xs, Gs and Ls
        stage_x(X, Xs, i0, n, D, xld);
        __syncthreads();
        {
            const f32x16 acc = zt_tile(wrow, Xs + il * xld + wave * kq, kq, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) Zs[wave * PROBE_TILE + acc_row(r, h) * 33 + il] = acc[r];
        }
        __syncthreads();
        if (wave == 0) {
            const int ig = i0 + il;
            const long long y = labels[min(ig, n - 1)];
            const bool live = ig < n && y >= 0 && y < C;
            const float wi = live ? (class_weight ? class_weight[y] : 1.f) : 0.f;
            float z[16];
            float m = NEG_BIG, zy = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = acc_row(r, h);
                const float* zp = Zs + c * 33 + il;
                z[r] = ((zp[0] + zp[PROBE_TILE]) + (zp[2 * PROBE_TILE] + zp[3 * PROBE_TILE])) + bc[r];
                if (c < C) {
                    m = fmaxf(m, z[r]);
                    if (c == y) zy = z[r];
                }
            }
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                z[r] = acc_row(r, h) < C ? expf(z[r] - m) : 0.f;
                s += z[r];
            }
            s += __shfl_xor(s, 32, 64);      // a + b == b + a: both halves hold the same bits
            zy += __shfl_xor(zy, 32, 64);    // the label's class sits in one half, the other adds 0
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = acc_row(r, h);
                float g = 0.f;
                if (live && c < C) g = wi * (z[r] / s - (c == y ? 1.f : 0.f));
                Gs[il * 33 + c] = g;
            }
            if (h == 0) Ls[il] = live ? wi * ((m + logf(s)) - zy) : 0.f;
        }
        __syncthreads();
        // second product: A[m = c][k = i] = G[i][c], B[k = i][n = d] = X[i][d]; half h takes the rows i = 2 kk + h
        // (kk is a real loop: unrolled whole, the compiler hoists all 16 (1 + NDT) LDS loads and spills at NDT = 8)
#pragma unroll 2
        for (int kk = 0; kk < 16; ++kk) {
            const int i = 2 * kk + h;
            const float a = Gs[i * 33 + il];
            const float* xrow = Xs + i * xld + wave * 32 + il;
#pragma unroll
            for (int t = 0; t < NDT; ++t)
                if (wave + 4 * t < ndtiles) dacc[t] = mfma_f32(a, xrow[128 * t], dacc[t]);
        }
        if (wave == 3) {
            if (lane < 32) {
                for (int i = 0; i < CLIP_ROWS; ++i) db += Gs[i * 33 + lane];
            } else if (lane == 32) {
                for (int i = 0; i < CLIP_ROWS; ++i) loss += (double)Ls[i];
            }
        }
    }

    // the partial: lane holds column d = dt*32 + il of the classes acc_row(r,h); every element has one owner
    unsigned char* base = partials + (size_t)blockIdx.x * stride;
    float* pw = reinterpret_cast<float*>(base + 8);
#pragma unroll
    for (int t = 0; t < NDT; ++t) {
        const int dt = wave + 4 * t;
        if (dt < ndtiles) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = acc_row(r, h);
                if (c < C) pw[(size_t)c * (D + 1) + dt * 32 + il] = dacc[t][r];
            }
        }
    }
    if (wave == 3) {
        if (lane < C) pw[(size_t)lane * (D + 1) + D] = db;          // C <= 32: lanes of the lower half
        if (lane == 32) *reinterpret_cast<double*>(base) = loss;
    }
}

// out[e] = sum_g partials[g][e] in index order, fp64; e < E = C (D+1) the gradient, e == E the loss
__global__ __launch_bounds__(256) void probe_finalize_kernel(const unsigned char* __restrict__ partials, size_t stride, int G, int E,
                                                             double* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e > E) return;
    double s = 0.0;
    if (e < E) {
        for (int g = 0; g < G; ++g) s += (double)reinterpret_cast<const float*>(partials + (size_t)g * stride + 8)[e];
    } else {
        for (int g = 0; g < G; ++g) s += *reinterpret_cast<const double*>(partials + (size_t)g * stride);
    }
    out[e] = s;
}

// =============================================================================================
// C ABI
// =============================================================================================
// the grid: n_groups > 0 as asked, 0 = one workgroup per CU; never more workgroups than 32-row blocks
static inline int probe_groups(int n, int n_groups) {
    const int nblocks = cdiv(n, CLIP_ROWS);
    const int want = n_groups > 0 ? n_groups : mmg_cu_count_cached();
    return want < nblocks ? want : nblocks;
}

MMG_API int mmg_probe_rows_supported(int D, int C) {
    if (D < 32 || D % 32 != 0 || D > 1024 || C < 2 || C > PROBE_MAX_C) return 0;
    return probe_lds_bytes(D) <= (size_t)PROBE_LDS_LIMIT ? 1 : 0;
}

MMG_API long long mmg_probe_rows_partials_bytes(int n, int D, int C, int n_groups) {
    if (!mmg_probe_rows_supported(D, C) || n < 1 || n_groups < 0 || n_groups > PROBE_MAX_GROUPS) return 0;
    return (long long)probe_groups(n, n_groups) * (long long)probe_partial_stride(D, C);
}

template <int NDT>
static void launch_probe_rows_ndt(const float* X, const float* W, const float* b, const long long* labels, const float* cw, int n, int D,
                                  int C, int G, unsigned char* partials, size_t stride, hipStream_t stream) {
    const size_t shm = probe_lds_bytes(D);
    mmg_allow_lds(probe_rows_kernel<NDT>, shm);
    MMG_NOTE_KERNEL("probe_rows_kernel<%d>", NDT);
    hipLaunchKernelGGL(probe_rows_kernel<NDT>, dim3(G), dim3(CLIP_THREADS), shm, stream, X, W, b, labels, cw, n, D, C, G, partials, stride);
}

MMG_API int mmg_probe_rows(const float* X, const float* W, const float* b, const long long* labels, const float* class_weight, int n,
                           int D, int C, int n_groups, void* partials, double* out, hipStream_t stream) {
    const char* who = "mmg_probe_rows";
    MMG_CHECK_ARG(n >= 1, "%s: n=%d must be positive", who, n);
    MMG_CHECK_ARG(D >= 32 && D % 32 == 0 && D <= 1024, "%s: D=%d must be a multiple of 32 in [32,1024]", who, D);
    MMG_CHECK_ARG(C >= 2 && C <= PROBE_MAX_C, "%s: C=%d must be in [2,%d]", who, C, PROBE_MAX_C);
    MMG_CHECK_ARG(mmg_probe_rows_supported(D, C), "%s: D=%d is unsupported: the staged rows and the tiles need %zu bytes of LDS, above %d", who,
                  D, probe_lds_bytes(D), PROBE_LDS_LIMIT);
    MMG_CHECK_ARG(n_groups >= 0 && n_groups <= PROBE_MAX_GROUPS, "%s: n_groups=%d must be in [0,%d] (0 = one workgroup per CU)", who, n_groups,
                  PROBE_MAX_GROUPS);
    MMG_CHECK_ARG(X && W && b && labels && partials && out, "%s: null pointer", who);
    MMG_CHECK_ARG(((uintptr_t)partials & 7) == 0 && ((uintptr_t)out & 7) == 0, "%s: partials and out must be 8-byte aligned", who);
    MMG_CHECK_ARG((((uintptr_t)X | (uintptr_t)W) & 15) == 0, "%s: X and W must be 16-byte aligned", who);
    const int G = probe_groups(n, n_groups);
    const size_t stride = probe_partial_stride(D, C);
    unsigned char* part = static_cast<unsigned char*>(partials);
    const int ndt = (D + 127) / 128;
    if (ndt <= 1) launch_probe_rows_ndt<1>(X, W, b, labels, class_weight, n, D, C, G, part, stride, stream);
    else if (ndt == 2) launch_probe_rows_ndt<2>(X, W, b, labels, class_weight, n, D, C, G, part, stride, stream);
    else if (ndt <= 4) launch_probe_rows_ndt<4>(X, W, b, labels, class_weight, n, D, C, G, part, stride, stream);
    else launch_probe_rows_ndt<8>(X, W, b, labels, class_weight, n, D, C, G, part, stride, stream);
    MMG_LAUNCH_CHECK(who);
    const int E = C * (D + 1);
    hipLaunchKernelGGL(probe_finalize_kernel, dim3(cdiv(E + 1, 256)), dim3(256), 0, stream, part, stride, G, E, out);
    MMG_LAUNCH_CHECK(who);
    return 0;
}
