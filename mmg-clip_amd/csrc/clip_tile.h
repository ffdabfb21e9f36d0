// The rows-against-Y tile skeleton of the contrastive heads (clip_head.hip, averaged_head.hip, sigmoid_head.hip; retrieval_head.hip,
// topk_head.hip and probe_head.hip use stage_x / zt_tile): a workgroup owns 32
// local rows of X in LDS and streams 32-column tiles of Y, fp32 on v_mfma_f32_32x32x2_f32 issued "swapped" (A = Y tile, B = X tile)
// so that a lane holds ONE row i and 16 columns j.  Written once here: the log-sum-exp forward (rows_lse_fwd_kernel), the backward
// dX = s G Y with its two scalar gradients (rows_bwd_kernel) and their launchers.  A head supplies only a rule: where a row's label
// comes from (forward) or how a dot product becomes the weight g_ij (backward); the rules live next to their C ABI in the .hip files.
#pragma once
#include "common.h"

#define CLIP_ROWS 32
#define CLIP_THREADS 256
#define NEG_BIG (-1.0e30f)

// row index inside a 32x32 f32 MFMA accumulator: reg r of lane-half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 mfma_f32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// ---------------------------------------------------------------------------------------------
// Z^T tile: acc[reg] of lane (i = lane&31, h = lane>>5) = <Y[j0 + acc_row(reg,h)], X[i]>
// Xs: LDS image of the 32 local rows, row pitch xld floats.  yrow: this lane's (clamped) Y row.
// k order inside a step is arbitrary as long as A and B agree: half h takes k = 8c + 4h + e.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x16 zt_tile(const float* __restrict__ yrow, const float* Xs_row, int D, int h) {
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float4* yp = reinterpret_cast<const float4*>(yrow) + h;
    const float4* xp = reinterpret_cast<const float4*>(Xs_row) + h;
#pragma unroll 4
    for (int c = 0; c < D / 8; ++c) {
        const float4 yv = yp[2 * c];
        const float4 xv = xp[2 * c];
        acc = mfma_f32(yv.x, xv.x, acc);
        acc = mfma_f32(yv.y, xv.y, acc);
        acc = mfma_f32(yv.z, xv.z, acc);
        acc = mfma_f32(yv.w, xv.w, acc);
    }
    return acc;
}

// Stage the workgroup's 32 rows of X into LDS (rows beyond n_loc are clamped duplicates).
__device__ __forceinline__ void stage_x(const float* __restrict__ X, float* Xs, int i0, int n_loc, int D, int xld) {
    const int nvec = D / 4;
    for (int idx = threadIdx.x; idx < CLIP_ROWS * nvec; idx += CLIP_THREADS) {
        const int r = idx / nvec, c = idx - r * nvec;
        const int gr = min(i0 + r, n_loc - 1);
        const float4 v = reinterpret_cast<const float4*>(X + (size_t)gr * D)[c];
        *reinterpret_cast<float4*>(Xs + r * xld + 4 * c) = v;
    }
}

// Online-softmax merge (m, l) <- (m, l) (+) (m2, l2): running maximum m and sum l of exp(z - m) over two disjoint sets of columns.
__device__ __forceinline__ void lse_merge(float& m, float& l, float m2, float l2) {
    const float mn = fmaxf(m, m2);
    l = l * __expf(m - mn) + l2 * __expf(m2 - mn);
    m = mn;
}

// ---------------------------------------------------------------------------------------------
// Forward: per local row i, lse[i] = logsumexp_j(s <X_i, Y_j>) and pos[i] = s <X_i, Y_{label(i)}> (0 for a label outside [0,N)).
// Label = where a row's label comes from: the kernel argument `arg` it is read from, its integer `type` and
// `static type of(arg, int ig, int n_loc)` (ig may be >= n_loc: clamp a load).
// Optionally writes the logits.
// ---------------------------------------------------------------------------------------------
template <class Label, bool WRITE_LOGITS>
__global__ __launch_bounds__(CLIP_THREADS) void rows_lse_fwd_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ scale_ptr, typename Label::arg label, int n_loc,
    int N, int D, float* __restrict__ lse, float* __restrict__ pos, float* __restrict__ logits, int ldl) {
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
    const typename Label::type lab = Label::of(label, ig, n_loc);
    const int ntiles = (N + 31) / 32;
    for (int jt = wave; jt < ntiles; jt += 4) {
        const int j0 = jt * 32;
        const float* yrow = Y + (size_t)min(j0 + il, N - 1) * D;
        const f32x16 acc = zt_tile(yrow, Xs + il * xld, D, h);
        float z[16];
        float tmax = NEG_BIG;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + acc_row(r, h);
            z[r] = acc[r] * scale;
            if (j < N) {
                tmax = fmaxf(tmax, z[r]);
                if ((typename Label::type)j == lab) p = z[r];
            }
        }
        // the tile's sum is taken against the NEW maximum, so this step is not an lse_merge of two finished pairs
        const float mn = fmaxf(m, tmax);
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + acc_row(r, h);
            if (j < N) s += __expf(z[r] - mn);
        }
        l = l * __expf(m - mn) + s;
        m = mn;
        if (WRITE_LOGITS && ig < n_loc) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = j0 + 8 * q + 4 * h;
                float* dst = logits + (size_t)ig * ldl + j;
                if (j + 3 < N && ((ldl & 3) == 0)) {
                    *reinterpret_cast<float4*>(dst) = make_float4(z[4 * q], z[4 * q + 1], z[4 * q + 2], z[4 * q + 3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (j + e < N) dst[e] = z[4 * q + e];
                }
            }
        }
    }
    // combine the two lane halves (same row i, disjoint columns)
    lse_merge(m, l, __shfl_xor(m, 32, 64), __shfl_xor(l, 32, 64));
    p += __shfl_xor(p, 32, 64);
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
            lse_merge(mm, ll, red[(w * 32 + threadIdx.x) * 3 + 0], red[(w * 32 + threadIdx.x) * 3 + 1]);
            pp += red[(w * 32 + threadIdx.x) * 3 + 2];
        }
        lse[i0 + threadIdx.x] = mm + __logf(ll);
        pos[i0 + threadIdx.x] = pp;
    }
}

// ---------------------------------------------------------------------------------------------
// Backward of the rows: dX[i,:] (+)= s * sum_j g_ij Y[j,:],  dscale += sum_ij g_ij <X_i,Y_j>,  dbias += sum_ij g_ij
// (one float atomic per workgroup and scalar).  The accumulator registers of the Z^T tile are parked in LDS as the G tile and fed
// back as the A operand of the second product with no lane movement.  NDT = 32-wide d tiles per wave (D <= 128*NDT).
//
// Pair = the rule dot -> g_ij, a struct of the head's operands passed by value:
//   typename Pair::Row row(int ig, int n_loc) const         what lane's row ig needs once (its lse, label, key, weight, c_up);
//                                                           ig may be >= n_loc (clamp any load: such a row's pairs are never asked)
//   float g(const Row&, float dot, float scale, int j) const   the weight of a VALID pair (ig < n_loc, j < N), dot = <X_ig, Y_j>
//   static constexpr bool DSCALE, DBIAS                      which scalar gradients the rule has (the pointers may still be null)
//   static constexpr bool ACCUMULATE                         whether the entry point has the `accumulate` flavour of the dX store
//   static constexpr const char* NOTE                        the kernel note, a printf format taking NDT
// A padded pair (the tile helpers clamp rows >= n_loc and columns >= N to duplicates of the last valid one) is SELECTED to zero here,
// not by the rule: a sigmoid has no "minus infinity" that would make it vanish.
// ---------------------------------------------------------------------------------------------
template <class Pair, int NDT>
__global__ __launch_bounds__(CLIP_THREADS) void rows_bwd_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ scale_ptr, Pair pair, int n_loc, int N,
    int D, int accumulate, float* __restrict__ dX, float* __restrict__ dscale, float* __restrict__ dbias) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int xld = D + 4;
    float* Xs = smem;                      // [32][xld]
    float* Gs = smem + CLIP_ROWS * xld;    // [4 slots][32 j][33]
    float* red = Gs + 4 * 32 * 33;         // [2][4]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int il = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * CLIP_ROWS;
    const int ig = i0 + il;
    const float scale = *scale_ptr;

    stage_x(X, Xs, i0, n_loc, D, xld);
    __syncthreads();

    f32x16 dacc[NDT];
#pragma unroll
    for (int t = 0; t < NDT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[t][r] = 0.f;

    const typename Pair::Row row = pair.row(ig, n_loc);
    float ds = 0.f, db = 0.f;
    const int ntiles = (N + 31) / 32;
    const int ndtiles = D / 32;
    for (int jt0 = 0; jt0 < ntiles; jt0 += 4) {
        const int jt = jt0 + wave;
        float* Gw = Gs + wave * 32 * 33;
        if (jt < ntiles) {
            const int j0 = jt * 32;
            const float* yrow = Y + (size_t)min(j0 + il, N - 1) * D;
            const f32x16 acc = zt_tile(yrow, Xs + il * xld, D, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jl = acc_row(r, h);
                const int j = j0 + jl;
                float g = 0.f;
                if (j < N && ig < n_loc) {
                    g = pair.g(row, acc[r], scale, j);
                    if (Pair::DSCALE) ds += g * acc[r];
                    if (Pair::DBIAS) db += g;
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
            if (j0 < N) {
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
                            const float b = ycol[(size_t)min(j0 + jl, N - 1) * D];          // B[k=jl][d]  (G is 0 on a clamped row)
                            dacc[t] = mfma_f32(a, b, dacc[t]);
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
                    *dst = (Pair::ACCUMULATE && accumulate) ? *dst + v : v;
                }
            }
        }
    }
    if ((Pair::DSCALE && dscale) || (Pair::DBIAS && dbias)) {
        if (Pair::DSCALE) ds = wave_sum(ds);
        if (Pair::DBIAS) db = wave_sum(db);
        if (lane == 0) {
            red[wave] = ds;
            red[4 + wave] = db;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (Pair::DSCALE && dscale) atomicAdd(dscale, (red[0] + red[1]) + (red[2] + red[3]));
            if (Pair::DBIAS && dbias) atomicAdd(dbias, (red[4] + red[5]) + (red[6] + red[7]));
        }
    }
}

// =============================================================================================
// Host side shared by the heads' C ABI
// =============================================================================================
// `cols` names the column count in the message ("N", or "M" where the entry point calls it so)
static inline int rows_check_dims(const char* who, int n_loc, int N, int D, const char* cols = "N") {
    MMG_CHECK_ARG(n_loc > 0 && N > 0, "%s: n_loc=%d %s=%d must be positive", who, n_loc, cols, N);
    MMG_CHECK_ARG(D >= 32 && D % 32 == 0 && D <= 1024, "%s: D=%d must be a multiple of 32 in [32,1024]", who, D);
    return 0;
}

static inline size_t rows_lds_bytes(int D, int tail_floats) { return (size_t)(CLIP_ROWS * (D + 4) + tail_floats) * sizeof(float); }

template <class Label, bool WRITE_LOGITS>
static void launch_rows_lse_fwd(const float* X, const float* Y, const float* scale, typename Label::arg label, int n_loc, int N,
                                int D, float* lse, float* pos, float* logits, int ldl, hipStream_t stream) {
    const size_t shm = rows_lds_bytes(D, 4 * 32 * 3);
    mmg_allow_lds(rows_lse_fwd_kernel<Label, WRITE_LOGITS>, shm);
    MMG_NOTE_KERNEL(Label::NOTE, WRITE_LOGITS ? "true" : "false");
    hipLaunchKernelGGL((rows_lse_fwd_kernel<Label, WRITE_LOGITS>), dim3(cdiv(n_loc, CLIP_ROWS)), dim3(CLIP_THREADS), shm, stream, X, Y,
                       scale, label, n_loc, N, D, lse, pos, logits, ldl);
}

template <class Pair, int NDT>
static void launch_rows_bwd_ndt(const float* X, const float* Y, const float* scale, const Pair& pair, int n_loc, int N, int D,
                                int accumulate, float* dX, float* dscale, float* dbias, hipStream_t stream) {
    const size_t shm = rows_lds_bytes(D, 4 * 32 * 33 + 8);
    mmg_allow_lds(rows_bwd_kernel<Pair, NDT>, shm);
    MMG_NOTE_KERNEL(Pair::NOTE, NDT);
    hipLaunchKernelGGL((rows_bwd_kernel<Pair, NDT>), dim3(cdiv(n_loc, CLIP_ROWS)), dim3(CLIP_THREADS), shm, stream, X, Y, scale, pair,
                       n_loc, N, D, accumulate, dX, dscale, dbias);
}

// The one NDT dispatch of the heads.  The caller checks the launch (MMG_LAUNCH_CHECK under its own name).
template <class Pair>
static void launch_rows_bwd(const float* X, const float* Y, const float* scale, const Pair& pair, int n_loc, int N, int D,
                            int accumulate, float* dX, float* dscale, float* dbias, hipStream_t stream) {
    const int ndt = (D + 127) / 128;
    if (ndt <= 1) launch_rows_bwd_ndt<Pair, 1>(X, Y, scale, pair, n_loc, N, D, accumulate, dX, dscale, dbias, stream);
    else if (ndt == 2) launch_rows_bwd_ndt<Pair, 2>(X, Y, scale, pair, n_loc, N, D, accumulate, dX, dscale, dbias, stream);
    else if (ndt <= 4) launch_rows_bwd_ndt<Pair, 4>(X, Y, scale, pair, n_loc, N, D, accumulate, dX, dscale, dbias, stream);
    else launch_rows_bwd_ndt<Pair, 8>(X, Y, scale, pair, n_loc, N, D, accumulate, dX, dscale, dbias, stream);
}
