// AveragedMedicalCLIPLoss from the (gathered) normalised embeddings, without an [n,N] logit matrix in HBM
// (reference mmgclip/loss/losses.py:164-216).
//
// The reference averages columns of A = s I T^T per text cluster; by linearity Abar[i,c] = s <I_i, Tbar_c> with Tbar_c the mean
// of the text embeddings of cluster c, so CE(Abar, c) is a rows-softmax of I against the [k,D] centroid matrix with a label per
// row.  The text side is CE(s T I^T, c) as the reference writes it (:213): row j has target column c(j).  Both are "rows of X
// against Y with a label per row"; the four gradient products dX = s g Y take two shapes of weight matrix g (ROW / COL below).
// Both run on the tile skeleton of clip_tile.h (rows_lse_fwd_kernel, rows_bwd_kernel); this file holds the label source and the
// two pair rules, next to the C ABI.
#include "clip_tile.h"

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
// label(r) = row_label[r]   (pos = 0 for a label outside [0,M))
struct RowLabel {
    using arg = const long long* __restrict__;
    using type = long long;
    static constexpr const char* NOTE = "rows_lse_fwd_kernel<RowLabel, %s>";
    static __device__ __forceinline__ long long of(arg row_label, int ig, int n_loc) { return row_label[min(ig, n_loc - 1)]; }
};

// lse[r] = logsumexp_m(s <X_r, Y_m>), pos[r] = s <X_r, Y_{row_label[r]}>
MMG_API int mmg_clip_labelled_rows_fwd(const float* X, const float* Y, const float* scale, const long long* row_label, int n_loc,
                                       int M, int D, float* lse, float* pos, hipStream_t stream) {
    if (rows_check_dims("mmg_clip_labelled_rows_fwd", n_loc, M, D, "M")) return 1;
    MMG_CHECK_ARG(X && Y && scale && row_label && lse && pos, "mmg_clip_labelled_rows_fwd: null pointer");
    launch_rows_lse_fwd<RowLabel, false>(X, Y, scale, row_label, n_loc, M, D, lse, pos, nullptr, 0, stream);
    MMG_LAUNCH_CHECK("mmg_clip_labelled_rows_fwd");
    return 0;
}

// Pair rules of rows_bwd_kernel (clip_tile.h) for labelled rows, with z[r,m] = s <X_r, Y_m> and c_up = coef * gout:
//   ROW : g[r,m] = c_up * (exp(z[r,m] - lse[r]) - [m == label[r]])                    lse, label: [n_loc]
//         (the rows' own softmax);  dscale += sum g[r,m] <X_r, Y_m>
//   COL : g[r,m] = c_up * w[r] * (exp(z[r,m] - lse[m]) - [label[m] == key[r]])        lse, label: [M]
//         (the softmax of the TRANSPOSED problem, whose rows are the M rows of Y);  key[r] = row_key ? row_key[r] : key_off + r,
//         w[r] = counts ? 1 / counts[key[r]] : 1;  no dscale (every softmax element is counted once, by its ROW product)
struct LabelledRowPair {
    static constexpr bool DSCALE = true, DBIAS = false, ACCUMULATE = true;
    static constexpr const char* NOTE = "rows_bwd_kernel<LabelledRowPair, %d>";
    const float* lse;
    const long long* label;
    const float* gout;
    float coef;
    struct Row {
        float lr, c_up;
        long long lab;
    };
    __device__ __forceinline__ Row row(int ig, int n_loc) const {
        const int igc = min(ig, n_loc - 1);
        return {lse[igc], coef * (gout ? *gout : 1.0f), label[igc]};
    }
    __device__ __forceinline__ float g(const Row& w, float dot, float scale, int j) const {
        float g = __expf(dot * scale - w.lr);
        if ((long long)j == w.lab) g -= 1.0f;
        return g * w.c_up;
    }
};

struct LabelledColPair {
    static constexpr bool DSCALE = false, DBIAS = false, ACCUMULATE = true;
    static constexpr const char* NOTE = "rows_bwd_kernel<LabelledColPair, %d>";
    const float* lse;
    const long long *label, *row_key;
    int key_off;
    const int* counts;
    int n_counts;
    const float* gout;
    float coef;
    struct Row {
        long long key;
        float c_up;
    };
    __device__ __forceinline__ Row row(int ig, int n_loc) const {
        const int igc = min(ig, n_loc - 1);
        const long long rk = row_key ? row_key[igc] : (long long)key_off + igc;
        float c_up = coef * (gout ? *gout : 1.0f);
        if (counts) c_up *= 1.0f / (float)((rk >= 0 && rk < n_counts) ? counts[rk] : 1);
        return {rk, c_up};
    }
    __device__ __forceinline__ float g(const Row& w, float dot, float scale, int j) const {
        float g = __expf(dot * scale - lse[j]);
        if (label[j] == w.key) g -= 1.0f;
        return g * w.c_up;
    }
};

MMG_API int mmg_clip_labelled_rows_bwd_row(const float* X, const float* Y, const float* scale, const float* lse_row,
                                           const long long* row_label, const float* gout, float coef, int n_loc, int M, int D,
                                           int accumulate, float* dX, float* dscale, hipStream_t stream) {
    if (rows_check_dims("mmg_clip_labelled_rows_bwd_row", n_loc, M, D, "M")) return 1;
    MMG_CHECK_ARG(X && Y && scale && lse_row && row_label && dX, "mmg_clip_labelled_rows_bwd_row: null pointer");
    launch_rows_bwd(X, Y, scale, LabelledRowPair{lse_row, row_label, gout, coef}, n_loc, M, D, accumulate, dX, dscale, nullptr, stream);
    MMG_LAUNCH_CHECK("mmg_clip_labelled_rows_bwd_row");
    return 0;
}

MMG_API int mmg_clip_labelled_rows_bwd_col(const float* X, const float* Y, const float* scale, const float* lse_col,
                                           const long long* col_label, const long long* row_key, int key_off, const int* counts,
                                           int n_counts, const float* gout, float coef, int n_loc, int M, int D, int accumulate,
                                           float* dX, hipStream_t stream) {
    if (rows_check_dims("mmg_clip_labelled_rows_bwd_col", n_loc, M, D, "M")) return 1;
    MMG_CHECK_ARG(X && Y && scale && lse_col && col_label && dX, "mmg_clip_labelled_rows_bwd_col: null pointer");
    MMG_CHECK_ARG(!counts || (row_key && n_counts > 0), "mmg_clip_labelled_rows_bwd_col: counts need row_key and n_counts=%d > 0",
                  n_counts);
    launch_rows_bwd(X, Y, scale, LabelledColPair{lse_col, col_label, row_key, key_off, counts, n_counts, gout, coef}, n_loc, M, D,
                    accumulate, dX, nullptr, nullptr, stream);
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
