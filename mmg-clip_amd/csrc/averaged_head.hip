// AveragedMedicalCLIPLoss from the (gathered) normalised embeddings, without an [n,N] logit matrix in HBM
// (reference mmgclip/loss/losses.py:164-216).
//
// The reference averages columns of A = s I T^T per text cluster; by linearity Abar[i,c] = s <I_i, Tbar_c> with Tbar_c the mean
// of the text embeddings of cluster c, so CE(Abar, c) is a rows-softmax of I against the [k,D] centroid matrix with a label per
// row.  The text side is CE(s T I^T, c) as the reference writes it (:213): row j has target column c(j).  Both are "rows of X
// against Y with a label per row"; the four gradient products dX = s g Y take two shapes of weight matrix g (ROW / COL below).
// Tiling as clip_head.hip: 32 local rows in LDS, 32-column tiles of Y streamed, four waves, fp32 v_mfma_f32_32x32x2_f32,
// the G tile fed back as the A operand of the second product.
#include "clip_tile.h"

// ---------------------------------------------------------------------------------------------
// Forward: lse[r] = logsumexp_m(s <X_r, Y_m>), pos[r] = s <X_r, Y_{row_label[r]}>   (pos = 0 for a label outside [0,M))
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CLIP_THREADS) void labelled_rows_fwd_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ scale_ptr,
    const long long* __restrict__ row_label, int n_loc, int M, int D, float* __restrict__ lse, float* __restrict__ pos) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int xld = D + 4;
    float* Xs = smem;                       // [32][xld]
    float* red = smem + CLIP_ROWS * xld;    // [4 waves][32 rows][3] (m, l, pos)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int il = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * CLIP_ROWS;
    const int ig = i0 + il;
    const float scale = *scale_ptr;

    stage_x(X, Xs, i0, n_loc, D, xld);
    __syncthreads();

    float m = NEG_BIG, l = 0.f, p = 0.f;
    const long long lab = row_label[min(ig, n_loc - 1)];
    const int ntiles = (M + 31) / 32;
    for (int jt = wave; jt < ntiles; jt += 4) {
        const int j0 = jt * 32;
        const float* yrow = Y + (size_t)min(j0 + il, M - 1) * D;
        const f32x16 acc = zt_tile(yrow, Xs + il * xld, D, h);
        float z[16];
        float tmax = NEG_BIG;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + acc_row(r, h);
            z[r] = acc[r] * scale;
            if (j < M) {
                tmax = fmaxf(tmax, z[r]);
                if ((long long)j == lab) p = z[r];
            }
        }
        const float mn = fmaxf(m, tmax);
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + acc_row(r, h);
            if (j < M) s += __expf(z[r] - mn);
        }
        l = l * __expf(m - mn) + s;
        m = mn;
    }
    // combine the two lane halves (same row, disjoint columns)
    {
        const float m2 = __shfl_xor(m, 32, 64), l2 = __shfl_xor(l, 32, 64), p2 = __shfl_xor(p, 32, 64);
        const float mn = fmaxf(m, m2);
        l = l * __expf(m - mn) + l2 * __expf(m2 - mn);
        m = mn;
        p += p2;
    }
    if (h == 0) {
        red[(wave * 32 + il) * 3 + 0] = m;
        red[(wave * 32 + il) * 3 + 1] = l;
        red[(wave * 32 + il) * 3 + 2] = p;
    }
    __syncthreads();
    if (threadIdx.x < 32 && i0 + threadIdx.x < n_loc) {
        float mm = NEG_BIG, ll = 0.f, pp = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float m2 = red[(w * 32 + threadIdx.x) * 3 + 0], l2 = red[(w * 32 + threadIdx.x) * 3 + 1];
            const float mn = fmaxf(mm, m2);
            ll = ll * __expf(mm - mn) + l2 * __expf(m2 - mn);
            mm = mn;
            pp += red[(w * 32 + threadIdx.x) * 3 + 2];
        }
        lse[i0 + threadIdx.x] = mm + __logf(ll);
        pos[i0 + threadIdx.x] = pp;
    }
}

// ---------------------------------------------------------------------------------------------
// Backward of labelled rows: dX[r,:] (+)= s * sum_m g[r,m] Y[m,:], with z[r,m] = s <X_r, Y_m> and c_up = coef * gout
//   ROW : g[r,m] = c_up * (exp(z[r,m] - lse[r]) - [m == label[r]])                    lse, label: [n_loc]
//         (the rows' own softmax);  dscale += sum g[r,m] <X_r, Y_m>
//   COL : g[r,m] = c_up * w[r] * (exp(z[r,m] - lse[m]) - [label[m] == key[r]])        lse, label: [M]
//         (the softmax of the TRANSPOSED problem, whose rows are the M rows of Y);  key[r] = row_key ? row_key[r] : key_off + r,
//         w[r] = counts ? 1 / counts[key[r]] : 1;  no dscale (every softmax element is counted once, by its ROW product)
// NDT = 32-wide d tiles per wave (D <= 128*NDT).
// ---------------------------------------------------------------------------------------------
template <bool COL, int NDT>
__global__ __launch_bounds__(CLIP_THREADS) void labelled_rows_bwd_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ scale_ptr,
    const float* __restrict__ lse, const long long* __restrict__ label, const long long* __restrict__ row_key, int key_off,
    const int* __restrict__ counts, int n_counts, const float* __restrict__ gout, float coef, int n_loc, int M, int D,
    int accumulate, float* __restrict__ dX, float* __restrict__ dscale) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int xld = D + 4;
    float* Xs = smem;                      // [32][xld]
    float* Gs = smem + CLIP_ROWS * xld;    // [4 slots][32 j][33]
    float* red = Gs + 4 * 32 * 33;         // [4]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int il = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * CLIP_ROWS;
    const int ig = i0 + il;
    const int igc = min(ig, n_loc - 1);
    const float scale = *scale_ptr;
    float c_up = coef * (gout ? *gout : 1.0f);

    stage_x(X, Xs, i0, n_loc, D, xld);
    __syncthreads();

    f32x16 dacc[NDT];
#pragma unroll
    for (int t = 0; t < NDT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[t][r] = 0.f;

    // per-row constants of this lane's row: ROW - its lse and label; COL - its key and weight
    float lr = 0.f;
    long long rk;
    if (COL) {
        rk = row_key ? row_key[igc] : (long long)key_off + igc;
        if (counts) c_up *= 1.0f / (float)((rk >= 0 && rk < n_counts) ? counts[rk] : 1);
    } else {
        lr = lse[igc];
        rk = label[igc];
    }
    float ds = 0.f;
    const int ntiles = (M + 31) / 32;
    const int ndtiles = D / 32;
    for (int jt0 = 0; jt0 < ntiles; jt0 += 4) {
        const int jt = jt0 + wave;
        float* Gw = Gs + wave * 32 * 33;
        if (jt < ntiles) {
            const int j0 = jt * 32;
            const float* yrow = Y + (size_t)min(j0 + il, M - 1) * D;
            const f32x16 acc = zt_tile(yrow, Xs + il * xld, D, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jl = acc_row(r, h);
                const int j = j0 + jl;
                float g = 0.f;
                if (j < M && ig < n_loc) {
                    const float z = acc[r] * scale;
                    if (COL) {
                        g = __expf(z - lse[j]);
                        if (label[j] == rk) g -= 1.0f;
                    } else {
                        g = __expf(z - lr);
                        if ((long long)j == rk) g -= 1.0f;
                    }
                    g *= c_up;
                    ds += g * acc[r];
                }
                Gw[jl * 33 + il] = g;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) Gw[acc_row(r, h) * 33 + il] = 0.f;
        }
        __syncthreads();
        // second product: every wave takes its d tiles over the 4 freshly written G tiles
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j0 = (jt0 + s) * 32;
            if (j0 < M) {
                const float* Gsl = Gs + s * 32 * 33;
#pragma unroll
                for (int t = 0; t < NDT; ++t) {
                    const int dt = wave + 4 * t;
                    if (dt < ndtiles) {
                        const float* ycol = Y + dt * 32 + il;
#pragma unroll
                        for (int kk = 0; kk < 16; ++kk) {
                            const int jl = 2 * kk + h;
                            const float a = Gsl[jl * 33 + il];                             // A[i][k=jl]
                            const float b = ycol[(size_t)min(j0 + jl, M - 1) * D];          // B[k=jl][d]
                            dacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, dacc[t], 0, 0, 0);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    // dX tile: lane holds column d = dt*32 + il, rows acc_row(r,h); every element has one owner, so accumulating is a plain add
#pragma unroll
    for (int t = 0; t < NDT; ++t) {
        const int dt = wave + 4 * t;
        if (dt < ndtiles) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + acc_row(r, h);
                if (i < n_loc) {
                    float* dst = dX + (size_t)i * D + dt * 32 + il;
                    const float v = dacc[t][r] * scale;
                    *dst = accumulate ? *dst + v : v;
                }
            }
        }
    }
    if (!COL && dscale) {
        ds = wave_sum(ds);
        if (lane == 0) red[wave] = ds;
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(dscale, red[0] + red[1] + red[2] + red[3]);
    }
}

// ---------------------------------------------------------------------------------------------
// Cluster centroids: out[c,:] = mean of T[j,:] over {j : labels[j] == c}, [N,D] -> [k,D].  One wave per cluster walks the labels
// 64 at a time and adds the member rows in ascending j: a fixed order and no float atomics, so every rank (and every run) that
// holds the same gathered bits gets the same centroid bits.  A cluster without members gives a zero row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cluster_centroids_kernel(const float* __restrict__ T, const long long* __restrict__ labels,
                                                                int N, int D, int k, float* __restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + wave;
    if (c >= k) return;
    float acc[16];                          // D <= 1024: column lane + 64 t
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0.f;
    int cnt = 0;
    for (int j0 = 0; j0 < N; j0 += 64) {
        const int j = j0 + lane;
        const bool mine = j < N && labels[j] == (long long)c;
        unsigned long long mask = __ballot(mine);
        cnt += __popcll(mask);
        while (mask) {
            const int jj = j0 + __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const float* row = T + (size_t)jj * D;
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (lane + 64 * t < D) acc[t] += row[lane + 64 * t];
        }
    }
    const float div = (float)max(cnt, 1);
#pragma unroll
    for (int t = 0; t < 16; ++t)
        if (lane + 64 * t < D) out[(size_t)c * D + lane + 64 * t] = acc[t] / div;
}

// =============================================================================================
// C ABI
// =============================================================================================
static int labelled_check_dims(const char* who, int n_loc, int M, int D) {
    MMG_CHECK_ARG(n_loc > 0 && M > 0, "%s: n_loc=%d M=%d must be positive", who, n_loc, M);
    MMG_CHECK_ARG(D >= 32 && D % 32 == 0 && D <= 1024, "%s: D=%d must be a multiple of 32 in [32,1024]", who, D);
    return 0;
}

MMG_API int mmg_clip_labelled_rows_fwd(const float* X, const float* Y, const float* scale, const long long* row_label, int n_loc,
                                       int M, int D, float* lse, float* pos, hipStream_t stream) {
    if (labelled_check_dims("mmg_clip_labelled_rows_fwd", n_loc, M, D)) return 1;
    MMG_CHECK_ARG(X && Y && scale && row_label && lse && pos, "mmg_clip_labelled_rows_fwd: null pointer");
    const size_t shm = (size_t)(CLIP_ROWS * (D + 4) + 4 * 32 * 3) * sizeof(float);
    mmg_allow_lds(labelled_rows_fwd_kernel, shm);
    hipLaunchKernelGGL(labelled_rows_fwd_kernel, dim3(cdiv(n_loc, CLIP_ROWS)), dim3(CLIP_THREADS), shm, stream, X, Y, scale,
                       row_label, n_loc, M, D, lse, pos);
    MMG_LAUNCH_CHECK("mmg_clip_labelled_rows_fwd");
    return 0;
}

template <bool COL>
static void launch_labelled_bwd(const float* X, const float* Y, const float* scale, const float* lse, const long long* label,
                                const long long* row_key, int key_off, const int* counts, int n_counts, const float* gout,
                                float coef, int n_loc, int M, int D, int accumulate, float* dX, float* dscale,
                                hipStream_t stream) {
    const size_t shm = (size_t)(CLIP_ROWS * (D + 4) + 4 * 32 * 33 + 4) * sizeof(float);
    const dim3 grid(cdiv(n_loc, CLIP_ROWS));
    const int ndt = (D + 127) / 128;
#define LAUNCH_LBWD(NDT)                                                                                                \
    do {                                                                                                                \
        mmg_allow_lds(labelled_rows_bwd_kernel<COL, NDT>, shm);                                                         \
        hipLaunchKernelGGL((labelled_rows_bwd_kernel<COL, NDT>), grid, dim3(CLIP_THREADS), shm, stream, X, Y, scale,    \
                           lse, label, row_key, key_off, counts, n_counts, gout, coef, n_loc, M, D, accumulate, dX,     \
                           dscale);                                                                                     \
    } while (0)
    if (ndt <= 1) LAUNCH_LBWD(1);
    else if (ndt == 2) LAUNCH_LBWD(2);
    else if (ndt <= 4) LAUNCH_LBWD(4);
    else LAUNCH_LBWD(8);
#undef LAUNCH_LBWD
}

MMG_API int mmg_clip_labelled_rows_bwd_row(const float* X, const float* Y, const float* scale, const float* lse_row,
                                           const long long* row_label, const float* gout, float coef, int n_loc, int M, int D,
                                           int accumulate, float* dX, float* dscale, hipStream_t stream) {
    if (labelled_check_dims("mmg_clip_labelled_rows_bwd_row", n_loc, M, D)) return 1;
    MMG_CHECK_ARG(X && Y && scale && lse_row && row_label && dX, "mmg_clip_labelled_rows_bwd_row: null pointer");
    launch_labelled_bwd<false>(X, Y, scale, lse_row, row_label, nullptr, 0, nullptr, 0, gout, coef, n_loc, M, D, accumulate, dX,
                               dscale, stream);
    MMG_LAUNCH_CHECK("mmg_clip_labelled_rows_bwd_row");
    return 0;
}

MMG_API int mmg_clip_labelled_rows_bwd_col(const float* X, const float* Y, const float* scale, const float* lse_col,
                                           const long long* col_label, const long long* row_key, int key_off, const int* counts,
                                           int n_counts, const float* gout, float coef, int n_loc, int M, int D, int accumulate,
                                           float* dX, hipStream_t stream) {
    if (labelled_check_dims("mmg_clip_labelled_rows_bwd_col", n_loc, M, D)) return 1;
    MMG_CHECK_ARG(X && Y && scale && lse_col && col_label && dX, "mmg_clip_labelled_rows_bwd_col: null pointer");
    MMG_CHECK_ARG(!counts || (row_key && n_counts > 0), "mmg_clip_labelled_rows_bwd_col: counts need row_key and n_counts=%d > 0",
                  n_counts);
    launch_labelled_bwd<true>(X, Y, scale, lse_col, col_label, row_key, key_off, counts, n_counts, gout, coef, n_loc, M, D,
                              accumulate, dX, nullptr, stream);
    MMG_LAUNCH_CHECK("mmg_clip_labelled_rows_bwd_col");
    return 0;
}

MMG_API int mmg_cluster_centroids(const float* T, const long long* labels, int N, int D, int k, float* out, hipStream_t stream) {
    MMG_CHECK_ARG(T && labels && out, "mmg_cluster_centroids: null pointer");
    MMG_CHECK_ARG(N > 0 && N <= 16384 && k > 0 && k <= N, "mmg_cluster_centroids: N=%d (1..16384) k=%d (1..N)", N, k);
    MMG_CHECK_ARG(D >= 32 && D % 32 == 0 && D <= 1024, "mmg_cluster_centroids: D=%d must be a multiple of 32 in [32,1024]", D);
    hipLaunchKernelGGL(cluster_centroids_kernel, dim3(cdiv(k, 4)), dim3(256), 0, stream, T, labels, N, D, k, out);
    MMG_LAUNCH_CHECK("mmg_cluster_centroids");
    return 0;
}
