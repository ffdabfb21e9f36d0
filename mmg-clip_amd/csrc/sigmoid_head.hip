// Sigmoid pairwise loss (SigLIP, Zhai et al. 2023) from the (gathered) normalised embeddings, without an [n,N] matrix in HBM.
// The reference has no such loss; this is an additive head next to clip_head.hip / averaged_head.hip.
//
//   z_ij = s <X_i, Y_j> + b,   y_ij = +1 for a positive pair and -1 otherwise,   u_ij = -y_ij z_ij
//   row_loss[i] = sum_j softplus(u_ij)                       g_ij = coef * gout * (-y_ij) * sigmoid(u_ij)
//   positive: col_label == NULL ? j == diag_off + i : col_label[j] == row_key[i]
//
// Every pair stands alone: there is no row normaliser to carry from the forward to the backward, so the backward recomputes z and
// needs nothing but the operands.  Tiling as clip_tile.h has it: 32 local rows in LDS, 32-column tiles of Y streamed, four waves
// (one workgroup pass covers 4 x 32 = 128 columns), fp32 v_mfma_f32_32x32x2_f32; the backward is rows_bwd_kernel under the rule
// SigmoidPair.  The tile helpers clamp rows >= n_loc and columns >= N to duplicates of the last valid one; a sigmoid has no
// "minus infinity" that makes such a pair vanish for both signs of y, so a padded pair is SELECTED to zero: below in the forward,
// by the skeleton (not the rule) in the backward.
#include "clip_tile.h"

#define SIG_COLS_PER_PASS (4 * 32)

// e = exp(-|u|) in (0,1]: softplus(u) = max(u,0) + log1p(e), sigmoid(u) = u >= 0 ? 1/(1+e) : e/(1+e).  Finite for every finite u;
// at |u| = 128 e underflows to 0 and the two are exactly max(u,0) and [u >= 0].
// expf / log1pf are the accurate library forms (not the __expf of the softmax heads, whose relative error grows with |u|): the head is
// far from the step's critical path and the error model of tests/sigmoid_ref.py then has one constant, K_FN ulps per call.
__device__ __forceinline__ float sig_softplus(float u) { return fmaxf(u, 0.f) + log1pf(expf(-fabsf(u))); }
__device__ __forceinline__ float sig_sigmoid(float u) {
    const float e = expf(-fabsf(u));
    return (u >= 0.f ? 1.0f : e) / (1.0f + e);
}

// ---------------------------------------------------------------------------------------------
// Forward: row_loss[i] = sum_j softplus(-y_ij z_ij).  One owner per row, a fixed summation tree, no atomics.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CLIP_THREADS) void sigmoid_rows_fwd_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ scale_ptr, const float* __restrict__ bias_ptr,
    const long long* __restrict__ row_key, const long long* __restrict__ col_label, int n_loc, int N, int D, int diag_off,
    float* __restrict__ row_loss) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int xld = D + 4;
    float* Xs = smem;                       // [32][xld]
    float* red = smem + CLIP_ROWS * xld;    // [4 waves][32 rows]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int il = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * CLIP_ROWS;
    const int ig = i0 + il;
    const float scale = *scale_ptr, bias = *bias_ptr;

    stage_x(X, Xs, i0, n_loc, D, xld);
    __syncthreads();

    const long long rk = col_label ? row_key[min(ig, n_loc - 1)] : (long long)diag_off + ig;
    float acc_l = 0.f;
    const int ntiles = (N + 31) / 32;
    for (int jt = wave; jt < ntiles; jt += 4) {
        const int j0 = jt * 32;
        const float* yrow = Y + (size_t)min(j0 + il, N - 1) * D;
        const f32x16 acc = zt_tile(yrow, Xs + il * xld, D, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + acc_row(r, h);
            float sp = 0.f;
            if (j < N) {
                const float z = fmaf(acc[r], scale, bias);
                const bool positive = (col_label ? col_label[j] : (long long)j) == rk;
                sp = sig_softplus(positive ? -z : z);
            }
            acc_l += sp;
        }
    }
    acc_l += __shfl_xor(acc_l, 32, 64);     // the two lane halves: same row, disjoint columns
    if (h == 0) red[wave * 32 + il] = acc_l;
    __syncthreads();
    if (threadIdx.x < 32 && i0 + threadIdx.x < n_loc)
        row_loss[i0 + threadIdx.x] = (red[threadIdx.x] + red[32 + threadIdx.x]) + (red[64 + threadIdx.x] + red[96 + threadIdx.x]);
}

// =============================================================================================
// C ABI
// =============================================================================================
static int sigmoid_check(const char* who, const void* X, const void* Y, const void* scale, const void* bias, const void* row_key,
                         const void* col_label, int n_loc, int N, int D, const void* out) {
    if (rows_check_dims(who, n_loc, N, D)) return 1;
    MMG_CHECK_ARG(X && Y && scale && bias && out, "%s: null pointer", who);
    MMG_CHECK_ARG((row_key != nullptr) == (col_label != nullptr), "%s: row_key and col_label come together (or both NULL: the diagonal)", who);
    return 0;
}

MMG_API int mmg_sigmoid_rows_fwd(const float* X, const float* Y, const float* scale, const float* bias, const long long* row_key,
                                 const long long* col_label, int n_loc, int N, int D, int diag_off, float* row_loss,
                                 hipStream_t stream) {
    if (sigmoid_check("mmg_sigmoid_rows_fwd", X, Y, scale, bias, row_key, col_label, n_loc, N, D, row_loss)) return 1;
    const size_t shm = rows_lds_bytes(D, 4 * 32);
    mmg_allow_lds(sigmoid_rows_fwd_kernel, shm);
    MMG_NOTE_KERNEL("sigmoid_rows_fwd_kernel");
    hipLaunchKernelGGL(sigmoid_rows_fwd_kernel, dim3(cdiv(n_loc, CLIP_ROWS)), dim3(CLIP_THREADS), shm, stream, X, Y, scale, bias,
                       row_key, col_label, n_loc, N, D, diag_off, row_loss);
    MMG_LAUNCH_CHECK("mmg_sigmoid_rows_fwd");
    return 0;
}

// Pair rule of rows_bwd_kernel (clip_tile.h): g_ij = coef * gout * (-y_ij) * sigmoid(-y_ij z_ij); both scalars, dbias += sum g_ij
struct SigmoidPair {
    static constexpr bool DSCALE = true, DBIAS = true, ACCUMULATE = false;
    static constexpr const char* NOTE = "sigmoid_rows_bwd_kernel<%d>";
    const float* bias;
    const long long *row_key, *col_label;
    const float* gout;
    float coef;
    int diag_off;
    struct Row {
        long long key;
        float bias, c_up;
    };
    __device__ __forceinline__ Row row(int ig, int n_loc) const {
        return {col_label ? row_key[min(ig, n_loc - 1)] : (long long)diag_off + ig, *bias, coef * (gout ? *gout : 1.0f)};
    }
    __device__ __forceinline__ float g(const Row& w, float dot, float scale, int j) const {
        const float z = fmaf(dot, scale, w.bias);
        const bool positive = (col_label ? col_label[j] : (long long)j) == w.key;
        return positive ? -w.c_up * sig_sigmoid(-z) : w.c_up * sig_sigmoid(z);
    }
};

// dX[i,:] = s * sum_j g_ij Y[j,:];  dscale / dbias (may be null) are ACCUMULATED
MMG_API int mmg_sigmoid_rows_bwd(const float* X, const float* Y, const float* scale, const float* bias, const long long* row_key,
                                 const long long* col_label, const float* gout, float coef, int n_loc, int N, int D, int diag_off,
                                 float* dX, float* dscale, float* dbias, hipStream_t stream) {
    if (sigmoid_check("mmg_sigmoid_rows_bwd", X, Y, scale, bias, row_key, col_label, n_loc, N, D, dX)) return 1;
    launch_rows_bwd(X, Y, scale, SigmoidPair{bias, row_key, col_label, gout, coef, diag_off}, n_loc, N, D, 0, dX, dscale, dbias, stream);
    MMG_LAUNCH_CHECK("mmg_sigmoid_rows_bwd");
    return 0;
}
