// Retrieval ranks at validation: for every local query X_i, where its best positive stands among the negatives of the whole gallery Y,
// without an [n,N] score matrix in HBM and without a sort.  The reference has no such metric; this is an additive head next to
// clip_head.hip / averaged_head.hip / sigmoid_head.hip, on the tile skeleton of clip_tile.h with a rule that COUNTS instead of sums.
//
//   s_ij = <X_i, Y_j>   (no scale, no bias: a positive scale does not change a rank, and integer data stays exact)
//   positive: col_label == NULL ? j == diag_off + i : col_label[j] == row_key[i]                  (exactly sigmoid_head.hip's rule)
//   n_pos[i] = #positives,  best[i] = max over the positives of s_ij (-inf for none),
//   n_gt[i] = #negatives with s_ij > best[i],  n_eq[i] = #negatives with s_ij == best[i];   rank_i = 1 + n_gt + n_eq on the host
//
// Two sweeps over the Y tiles: the threshold `best` of a row is only known once every positive has been seen, so sweep 1 finds it and
// sweep 2 counts against it.  Both form s_ij through zt_tile - the same MFMA chain in the same k order on the same operands - so the
// value compared in sweep 2 has the bits of the value maximised in sweep 1; that is what gives `==` a meaning.  The price is the
// forward's MFMAs twice; the head runs once per validation epoch and is not tuned beyond that.
// Counts are integers, every row has one owner and the tree is fixed (16 columns of a tile per lane, a wave's tiles in order, the
// two lane halves, the four waves): bit-reproducible, and a row's results do not depend on which rows share its launch.
// The tile helpers clamp rows >= n_loc and columns >= N to duplicates of the last valid one: a padded column is never looked at
// (j < N below), a padded row is computed and not written.
#include <math.h>

#include "clip_tile.h"

__device__ __forceinline__ bool retrieval_positive(const long long* __restrict__ col_label, long long key, int j) {
    return (col_label ? col_label[j] : (long long)j) == key;
}

__global__ __launch_bounds__(CLIP_THREADS) void retrieval_rows_rank_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const long long* __restrict__ row_key,
    const long long* __restrict__ col_label, int n_loc, int N, int D, int diag_off, float* __restrict__ best, int* __restrict__ n_pos,
    int* __restrict__ n_gt, int* __restrict__ n_eq) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int xld = D + 4;
    float* Xs = smem;                                            // [32][xld]
    float* red_best = smem + CLIP_ROWS * xld;                    // [4 waves][32 rows]
    int* red_pos = reinterpret_cast<int*>(red_best + 4 * 32);    // [4 waves][32 rows]
    int* red_gt = red_pos + 4 * 32;
    int* red_eq = red_gt + 4 * 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int il = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * CLIP_ROWS;
    const int ig = i0 + il;

    stage_x(X, Xs, i0, n_loc, D, xld);
    __syncthreads();

    const long long key = col_label ? row_key[min(ig, n_loc - 1)] : (long long)diag_off + ig;
    const int ntiles = (N + 31) / 32;

    // ---- sweep 1: the best positive and the number of positives.  On the diagonal the workgroup's positives are the columns
    //      diag_off + i0 .. diag_off + i0 + 31, which meet one or two tiles; labelled positives may be anywhere
    int t_lo = 0, t_hi = ntiles - 1;
    if (!col_label) {
        t_lo = (diag_off + i0) / 32;
        t_hi = min((diag_off + i0 + 31) / 32, ntiles - 1);
    }
    float b = -INFINITY;
    int np = 0;
    for (int jt = t_lo + wave; jt <= t_hi; jt += 4) {
        const int j0 = jt * 32;
        const float* yrow = Y + (size_t)min(j0 + il, N - 1) * D;
        const f32x16 acc = zt_tile(yrow, Xs + il * xld, D, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + acc_row(r, h);
            if (j < N && retrieval_positive(col_label, key, j)) {
                b = fmaxf(b, acc[r]);
                ++np;
            }
        }
    }
    b = fmaxf(b, __shfl_xor(b, 32, 64));          // the two lane halves: same row, disjoint columns
    np += __shfl_xor(np, 32, 64);
    if (h == 0) {
        red_best[wave * 32 + il] = b;
        red_pos[wave * 32 + il] = np;
    }
    __syncthreads();
    // every lane takes its row's threshold back (a maximum and an integer sum: the order cannot matter, and it is fixed anyway)
    b = fmaxf(fmaxf(red_best[il], red_best[32 + il]), fmaxf(red_best[64 + il], red_best[96 + il]));

    // ---- sweep 2: the negatives above and at the threshold
    int gt = 0, eq = 0;
    for (int jt = wave; jt < ntiles; jt += 4) {
        const int j0 = jt * 32;
        const float* yrow = Y + (size_t)min(j0 + il, N - 1) * D;
        const f32x16 acc = zt_tile(yrow, Xs + il * xld, D, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + acc_row(r, h);
            if (j < N && !retrieval_positive(col_label, key, j)) {
                gt += acc[r] > b;
                eq += acc[r] == b;
            }
        }
    }
    gt += __shfl_xor(gt, 32, 64);
    eq += __shfl_xor(eq, 32, 64);
    if (h == 0) {
        red_gt[wave * 32 + il] = gt;
        red_eq[wave * 32 + il] = eq;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 32 && i0 + t < n_loc) {
        best[i0 + t] = fmaxf(fmaxf(red_best[t], red_best[32 + t]), fmaxf(red_best[64 + t], red_best[96 + t]));
        n_pos[i0 + t] = (red_pos[t] + red_pos[32 + t]) + (red_pos[64 + t] + red_pos[96 + t]);
        n_gt[i0 + t] = (red_gt[t] + red_gt[32 + t]) + (red_gt[64 + t] + red_gt[96 + t]);
        n_eq[i0 + t] = (red_eq[t] + red_eq[32 + t]) + (red_eq[64 + t] + red_eq[96 + t]);
    }
}

// =============================================================================================
// C ABI
// =============================================================================================
MMG_API int mmg_retrieval_rows_rank(const float* X, const float* Y, const long long* row_key, const long long* col_label, int n_loc,
                                    int N, int D, int diag_off, float* best, int* n_pos, int* n_gt, int* n_eq, hipStream_t stream) {
    const char* who = "mmg_retrieval_rows_rank";
    if (rows_check_dims(who, n_loc, N, D)) return 1;
    MMG_CHECK_ARG(X && Y && best && n_pos && n_gt && n_eq, "%s: null pointer", who);
    MMG_CHECK_ARG((row_key != nullptr) == (col_label != nullptr), "%s: row_key and col_label come together (or both NULL: the diagonal)", who);
    MMG_CHECK_ARG(col_label || (diag_off >= 0 && (long long)diag_off + n_loc <= N),
                  "%s: diagonal positives need 0 <= diag_off and diag_off + n_loc <= N (diag_off=%d n_loc=%d N=%d)", who, diag_off, n_loc, N);
    const size_t shm = rows_lds_bytes(D, 4 * 4 * 32);
    mmg_allow_lds(retrieval_rows_rank_kernel, shm);
    MMG_NOTE_KERNEL("retrieval_rows_rank_kernel");
    hipLaunchKernelGGL(retrieval_rows_rank_kernel, dim3(cdiv(n_loc, CLIP_ROWS)), dim3(CLIP_THREADS), shm, stream, X, Y, row_key, col_label,
                       n_loc, N, D, diag_off, best, n_pos, n_gt, n_eq);
    MMG_LAUNCH_CHECK(who);
    return 0;
}
