// Nearest-neighbour search over a gallery: for every local query X_i the k best columns of Y, without an [n,N] score matrix in HBM
// and without a sort of one.  The reference has no such search (its PromptClassifier scores a handful of prompts densely); this is an
// additive head next to retrieval_head.hip, on the tile skeleton of clip_tile.h with a rule that SELECTS instead of summing or counting.
//
//   s_ij = <X_i, Y_j>   (no scale, no bias: as retrieval_head.hip, so integer data stays exact and a pair's score has the same bits)
//   column j has the global index J = j_base + j;  excluded: exclude == 1 ? J == diag_off + i : exclude == 2 ? col_label[j] == row_key[i]
//   row i receives its k best admissible columns under the TOTAL order (score descending, then J ascending), padded with (-inf, -1).
//
// One sorted candidate list per (wave, row) in LDS, slot-major ([wave][slot][row]: the 32 rows of a slot fall into 32 banks).  A wave
// sweeps its tiles (jt = wave, wave + 4, ..); a lane holds one row and 16 columns, the upper lane half hands its 16 scores to the lower
// one (one cross-half exchange per register), and the lower lane alone tests all 32 against its list's k-th entry, kept in registers
// (one compare each, a bit mask of survivors), and then inserts the survivors alone.  A list therefore has ONE owner thread during
// the sweep: no atomics, no cross-lane memory traffic.
// After the sweep 32 threads each four-way-merge their row's lists and store.  Under `accumulate` wave 0's list starts as the list
// the buffers already hold (sorted, padded, over other columns), so the stored list is the top-k of the union.
// The order is total, so the result is unique: it cannot depend on the insertion order, on how the gallery is cut into launches
// (j_base / accumulate), on which rows share a launch or on the run.  FINITE inputs are assumed; NaN is not defined here.
// The tile helpers clamp rows >= n_loc and columns >= N to duplicates of the last valid one: a padded column is never admitted
// (j < N below), a padded row is computed and not written.
#include <math.h>

#include "clip_tile.h"

#define TOPK_MAX_K 32
#define TOPK_LDS_LIMIT 163840          // 160 KB of LDS per workgroup on gfx950

// (s, j) stands before (es, ej) in the order; ej < 0 is padding, which stands after every column.  (s, j) is a real column.
__device__ __forceinline__ bool topk_before(float s, int j, float es, int ej) { return ej < 0 || s > es || (s == es && j < ej); }

__device__ __forceinline__ bool topk_excluded(int exclude, const long long* __restrict__ col_label, long long key, int j, int j_base) {
    if (exclude == 1) return (long long)j_base + j == key;
    if (exclude == 2) return col_label[j] == key;
    return false;
}

// Insert (s, J) into the sorted list ls / li (slot pitch 32) when it beats the k-th entry (ts, tj), which is kept up to date.
__device__ __forceinline__ void topk_insert(float* ls, int* li, int k, float s, int J, float& ts, int& tj) {
    if (!topk_before(s, J, ts, tj)) return;
    int p = k - 1;
    while (p > 0) {
        const float es = ls[(p - 1) * 32];
        const int ej = li[(p - 1) * 32];
        if (!topk_before(s, J, es, ej)) break;
        ls[p * 32] = es;
        li[p * 32] = ej;
        --p;
    }
    ls[p * 32] = s;
    li[p * 32] = J;
    ts = ls[(k - 1) * 32];
    tj = li[(k - 1) * 32];
}

__global__ __launch_bounds__(CLIP_THREADS) void topk_rows_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, int n_loc, int N, int D, int k, int exclude,
    const long long* __restrict__ row_key, const long long* __restrict__ col_label, int diag_off, int j_base, int accumulate,
    float* __restrict__ scores, int* __restrict__ indices) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int xld = D + 4;
    float* Xs = smem;                                                  // [32][xld]
    float* Ls = smem + CLIP_ROWS * xld;                                // [4 waves][k slots][32 rows] scores
    int* Li = reinterpret_cast<int*>(Ls + 4 * k * 32);                 // [4 waves][k slots][32 rows] global indices
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int il = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * CLIP_ROWS;
    const int ig = i0 + il;

    stage_x(X, Xs, i0, n_loc, D, xld);

    // the list of (wave, row il): owned by the lower lane half.  Empty, or (wave 0, accumulate) what the buffers hold for this row
    float* ls = Ls + wave * k * 32 + il;
    int* li = Li + wave * k * 32 + il;
    float ts = -INFINITY;
    int tj = -1;
    if (h == 0) {
        const bool seed = accumulate && wave == 0 && ig < n_loc;
        for (int s = 0; s < k; ++s) {
            ls[s * 32] = seed ? scores[(size_t)ig * k + s] : -INFINITY;
            li[s * 32] = seed ? indices[(size_t)ig * k + s] : -1;
        }
        ts = ls[(k - 1) * 32];
        tj = li[(k - 1) * 32];
    }
    __syncthreads();

    const long long key = exclude == 2 ? row_key[min(ig, n_loc - 1)] : (long long)diag_off + ig;
    const int ntiles = (N + 31) / 32;
    for (int jt = wave; jt < ntiles; jt += 4) {
        const int j0 = jt * 32;
        const float* yrow = Y + (size_t)min(j0 + il, N - 1) * D;
        const f32x16 acc = zt_tile(yrow, Xs + il * xld, D, h);
        // candidate c of the row: c < 16 this lane's register c, c >= 16 the other half's register c - 16.  First ONE compare each
        // against the k-th entry (bit c of `live`), then the survivors alone are inserted: the wave walks as many insertions as its
        // busiest row has survivors, not 32.  (topk_insert tests again: the k-th entry moves while the survivors go in.)
        f32x16 oth;
        unsigned live = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            oth[r] = __shfl_xor(acc[r], 32, 64);                   // the same row's score of column acc_row(r, 1 - h)
            if (h == 0) {
                const int ja = j0 + acc_row(r, 0), jb = j0 + acc_row(r, 1);
                if (ja < N && topk_before(acc[r], j_base + ja, ts, tj) && !topk_excluded(exclude, col_label, key, ja, j_base)) live |= 1u << r;
                if (jb < N && topk_before(oth[r], j_base + jb, ts, tj) && !topk_excluded(exclude, col_label, key, jb, j_base))
                    live |= 1u << (16 + r);
            }
        }
        if (h == 0) {
            while (live) {
                const int c = __ffs(live) - 1;
                live &= live - 1;
                const int r = c & 15;
                float s = c < 16 ? acc[0] : oth[0];
#pragma unroll
                for (int q = 1; q < 16; ++q) s = r == q ? (c < 16 ? acc[q] : oth[q]) : s;
                topk_insert(ls, li, k, s, j_base + j0 + acc_row(r, c >> 4), ts, tj);
            }
        }
    }
    __syncthreads();

    // four-way merge of the row's lists: k picks, each the first of the four heads in the order
    const int t = threadIdx.x;
    if (t < 32 && i0 + t < n_loc) {
        int p[4] = {0, 0, 0, 0};
        float hs[4];
        int hj[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            hs[w] = Ls[w * k * 32 + t];
            hj[w] = Li[w * k * 32 + t];
        }
        float* so = scores + (size_t)(i0 + t) * k;
        int* io = indices + (size_t)(i0 + t) * k;
        for (int o = 0; o < k; ++o) {
            int bw = -1, bj = -1;
            float bs = -INFINITY;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (hj[w] >= 0 && topk_before(hs[w], hj[w], bs, bj)) {
                    bw = w;
                    bs = hs[w];
                    bj = hj[w];
                }
            }
            so[o] = bs;
            io[o] = bj;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (w == bw) {
                    ++p[w];
                    const bool more = p[w] < k;
                    hs[w] = more ? Ls[(w * k + p[w]) * 32 + t] : -INFINITY;
                    hj[w] = more ? Li[(w * k + p[w]) * 32 + t] : -1;
                }
            }
        }
    }
}

// =============================================================================================
// C ABI
// =============================================================================================
static inline size_t topk_lds_bytes(int D, int k) { return rows_lds_bytes(D, 4 * 32 * k * 2); }

MMG_API int mmg_topk_rows_supported(int D, int k) {
    if (D < 32 || D % 32 != 0 || D > 1024 || k < 1 || k > TOPK_MAX_K) return 0;
    return topk_lds_bytes(D, k) <= (size_t)TOPK_LDS_LIMIT ? 1 : 0;
}

MMG_API int mmg_topk_rows_lds_bytes(int D, int k) { return mmg_topk_rows_supported(D, k) ? (int)topk_lds_bytes(D, k) : 0; }

MMG_API int mmg_topk_rows(const float* X, const float* Y, int n_loc, int N, int D, int k, int exclude, const long long* row_key,
                          const long long* col_label, int diag_off, int j_base, int accumulate, float* scores, int* indices,
                          hipStream_t stream) {
    const char* who = "mmg_topk_rows";
    if (rows_check_dims(who, n_loc, N, D)) return 1;
    MMG_CHECK_ARG(k >= 1 && k <= TOPK_MAX_K, "%s: k=%d must be in [1,%d]", who, k, TOPK_MAX_K);
    MMG_CHECK_ARG(mmg_topk_rows_supported(D, k), "%s: D=%d with k=%d is unsupported: the staged rows and the lists need %zu bytes of LDS, above %d",
                  who, D, k, topk_lds_bytes(D, k), TOPK_LDS_LIMIT);
    MMG_CHECK_ARG(exclude >= 0 && exclude <= 2, "%s: exclude=%d must be 0 (none), 1 (diagonal) or 2 (labels)", who, exclude);
    MMG_CHECK_ARG(exclude == 2 || (!row_key && !col_label), "%s: row_key and col_label must be NULL unless exclude=2 (exclude=%d)", who, exclude);
    MMG_CHECK_ARG(exclude != 2 || (row_key && col_label), "%s: exclude=2 needs row_key and col_label", who);
    MMG_CHECK_ARG(exclude != 1 || diag_off >= 0, "%s: exclude=1 needs diag_off >= 0 (diag_off=%d)", who, diag_off);
    MMG_CHECK_ARG(j_base >= 0 && (long long)j_base + N <= 2147483647LL, "%s: j_base=%d must be >= 0 and j_base + N fit int32 (N=%d)", who, j_base, N);
    MMG_CHECK_ARG(X && Y && scores && indices, "%s: null pointer", who);
    const size_t shm = topk_lds_bytes(D, k);
    mmg_allow_lds(topk_rows_kernel, shm);
    MMG_NOTE_KERNEL("topk_rows_kernel");
    hipLaunchKernelGGL(topk_rows_kernel, dim3(cdiv(n_loc, CLIP_ROWS)), dim3(CLIP_THREADS), shm, stream, X, Y, n_loc, N, D, k, exclude, row_key,
                       col_label, diag_off, j_base, accumulate, scores, indices);
    MMG_LAUNCH_CHECK(who);
    return 0;
}
