// Zero-shot AUROC with bootstrap replicates, as exact integer pair counts on the i8 matrix cores (mmgclip/zeroshot_auroc.py).
// The reference scores AUROC on the host (sklearn) and bootstraps it as 1000 more host calls from an unseeded generator
// (evaluator.py:130-137); here a replicate is the SAME double sum with the resample's multiplicities as integer weights:
//
//   U2_b = sum_i sum_j w+[b][i] * w-[b][j] * g(s+_i, s-_j),   g = 2 [s+ > s-] + [s+ == s-],   AUROC_b = U2_b / (2 W+_b W-_b)
//
// T[i][b] = sum_j g(s+_i, s-_j) w-[b][j] is a GEMM whose left operand (entries 0, 1, 2) is formed in registers from two score
// vectors and never stored, on v_mfma_i32_32x32x32_i8 with an int32 accumulator; then U2_b = sum_i w+[b][i] T[i][b] in int64.
// No float is added anywhere: the result is exact, needs no sort and no [P,Nn] matrix.
//
// mmg_auroc_pairs, one workgroup = 32 positives (the MFMA rows) x 256 replicates (8 column tiles of 32), 4 waves that split the
// negatives (K) in chunks of 32: wave w takes chunks w, w + 4, ...
//   A fragment  lane (r = lane & 31, h = lane >> 5) holds g(s+_{i0 + r}, s-_{k0 + j}), j = 0..15, k0 = 32 chunk + 16 h, byte j;
//               its 16 negative scores are the same for the 32 lanes of a half (a broadcast load).  Built once per chunk (about
//               5 VALU operations per byte) and used against the 8 replicate tiles, so that the build sits under 8 MFMAs.
//   B fragment  the same lane holds w-[b0 + 32 tile + r][k0 + j], j = 0..15: 16 contiguous bytes of one replicate's weight row.
//               Both fragments give byte j of lane half h the same negative k0 + j, and A and B share one k map, which is all the
//               product needs; the one-hot cases of tests/test_auroc_gpu.py pin this.
//   C/D         column (replicate) = lane & 31, row (positive) = (reg & 3) + 8 (reg >> 2) + 4 h: the dtype-independent map.
// Blocking 1 row tile x 8 replicate tiles: the A build is the bound (VALU), not the weight stream, so the A fragment is what gets
// reused; the price is that the weight matrix is read once per 32 positives (from the Infinity Cache as long as the caller keeps a
// chunk of weights small enough: ZeroShotAUROC's default, max_weight_bytes, is 64 MiB).  8 x 16 = 128 accumulator registers plus 177 others as compiled: one wave per SIMD, 8 KiB of LDS.
// Rows >= P are computed on a clamped score and never added (guarded by i < P where w+ is applied); columns >= Nn get the
// score +inf, against which g = 0 for every finite s+, and the caller's zero weights there; replicates >= B load a zero fragment.
// Every (row block, replicate) has one owner and a fixed tree - 16 registers, the two lane halves, the four waves through LDS -
// and all of it is integer: bit-identical from run to run and however the positives are split over launches.
// int32 bound, enforced by the host: T <= 2 max_b sum_j w-[b][j] < 2^31.
//
// mmg_bootstrap_weights: replicate b's n draws, t' = 0..n-1, land on idx = (u * n) >> 32 with u = mmg_drop_bits(t', key_b),
// key_b = mmg_drop_key_bh(mmg_drop_key(seed, SITE_BOOTSTRAP), b) (dropout.h's hash).  The multiply-high maps 2^32 values onto n
// cells whose sizes differ by at most one: the bias is below n / 2^32 per value.  One workgroup owns one replicate and one tile of
// 8192 targets: it walks all n draws and counts those of its tile with integer LDS atomics (a sum of integers does not depend on
// the order), then narrows to int8.  No scratch, no memset, no global atomic.  A count above 127 is written as -128, which no
// count is; the host raises on any negative weight.
#include <math.h>

#include "common.h"
#include "dropout.h"

typedef __attribute__((ext_vector_type(16))) int i32x16;

#define AUROC_THREADS 256
#define AUROC_ROWS 32
#define AUROC_CT 8                       // replicate tiles of 32 per workgroup
#define AUROC_COLS (32 * AUROC_CT)
#define SITE_BOOTSTRAP 0x200u            // BERT's sites are 0..4 layers + 3, stochastic depth's the block numbers, augment's 0x100..0x105
#define BOOT_TILE 8192                   // targets per workgroup: 32 KiB of LDS counters
#define BOOT_OVERFLOW (-128)

// four values of g packed to bytes, lowest byte first
__device__ __forceinline__ int auroc_g4(float sp, float a, float b, float c, float d) {
    const unsigned ga = (unsigned)(sp > a) + (unsigned)(sp >= a), gb = (unsigned)(sp > b) + (unsigned)(sp >= b);
    const unsigned gc = (unsigned)(sp > c) + (unsigned)(sp >= c), gd = (unsigned)(sp > d) + (unsigned)(sp >= d);
    return (int)(ga | (gb << 8) | (gc << 16) | (gd << 24));
}

__global__ __launch_bounds__(AUROC_THREADS) void auroc_pairs_kernel(
    const float* __restrict__ s_pos, const float* __restrict__ s_neg, const signed char* __restrict__ w_pos, int ldw_pos,
    const signed char* __restrict__ w_neg, int ldw_neg, int P, int Nn, int B, long long* __restrict__ partial) {
    __shared__ long long red[4][AUROC_CT][32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * AUROC_ROWS;
    const int bbase = blockIdx.y * AUROC_COLS;
    const int nct = min(AUROC_CT, (B - bbase + 31) / 32);
    const float sp = s_pos[min(i0 + r, P - 1)];
    const int nchunks = (Nn + 31) / 32;
    const int kpad = (Nn + 15) & ~15;

    i32x16 acc[AUROC_CT];
#pragma unroll
    for (int ct = 0; ct < AUROC_CT; ++ct)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[ct][q] = 0;

    for (int c = wave; c < nchunks; c += 4) {
        const int k0 = c * 32 + 16 * h;
        float sn[16];
        if (k0 + 16 <= Nn) {
            const float4* p4 = reinterpret_cast<const float4*>(s_neg + k0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = p4[q];
                sn[4 * q] = v.x; sn[4 * q + 1] = v.y; sn[4 * q + 2] = v.z; sn[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) sn[j] = k0 + j < Nn ? s_neg[k0 + j] : INFINITY;
        }
        i32x4 a;
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = auroc_g4(sp, sn[4 * q], sn[4 * q + 1], sn[4 * q + 2], sn[4 * q + 3]);
        const bool kin = k0 < kpad;
#pragma unroll
        for (int ct = 0; ct < AUROC_CT; ++ct) {
            if (ct < nct) {                                     // (uniform over the workgroup)
                const int bb = bbase + ct * 32 + r;
                i32x4 bf = {0, 0, 0, 0};
                if (kin && bb < B) bf = *reinterpret_cast<const i32x4*>(w_neg + (size_t)bb * ldw_neg + k0);
                acc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bf, acc[ct], 0, 0, 0);
            }
        }
    }

    // U2 of this wave's share of K: w+ applied in int64, then the two lane halves (same replicate, disjoint rows)
#pragma unroll
    for (int ct = 0; ct < AUROC_CT; ++ct) {
        if (ct < nct) {
            const int bb = bbase + ct * 32 + r;
            long long v = 0;
            if (bb < B) {
                const signed char* wp = w_pos + (size_t)bb * ldw_pos;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int i = i0 + (q & 3) + 8 * (q >> 2) + 4 * h;
                    if (i < P) v += (long long)acc[ct][q] * (long long)wp[i];
                }
            }
            v += __shfl_xor(v, 32, 64);
            if (h == 0) red[wave][ct][r] = v;
        }
    }
    __syncthreads();
    const int ct = threadIdx.x >> 5, col = threadIdx.x & 31;
    const int bb = bbase + ct * 32 + col;
    if (ct < nct && bb < B)
        partial[(size_t)blockIdx.x * B + bb] = (red[0][ct][col] + red[1][ct][col]) + (red[2][ct][col] + red[3][ct][col]);
}

__global__ __launch_bounds__(256) void bootstrap_weights_kernel(unsigned key, int n, int b0, signed char* __restrict__ w, int ldw) {
    __shared__ int hist[BOOT_TILE];
    const int t0 = blockIdx.x * BOOT_TILE;
    const unsigned key_b = mmg_drop_key_bh(key, (unsigned)(b0 + (int)blockIdx.y));
    for (int c = threadIdx.x; c < BOOT_TILE; c += 256) hist[c] = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += 256) {
        const unsigned idx = (unsigned)(((unsigned long long)mmg_drop_bits((unsigned)t, key_b) * (unsigned long long)(unsigned)n) >> 32);
        const unsigned rel = idx - (unsigned)t0;
        if (rel < (unsigned)BOOT_TILE) atomicAdd(&hist[rel], 1);
    }
    __syncthreads();
    // four columns per thread and store (t0 and ldw are multiples of 4); columns n .. ldw-1 counted nothing and are written as 0
    signed char* row = w + (size_t)blockIdx.y * ldw;
    for (int c = 4 * threadIdx.x; c < BOOT_TILE && t0 + c < ldw; c += 4 * 256) {
        unsigned packed = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int v = hist[c + q];
            packed |= (unsigned)((v > 127 ? BOOT_OVERFLOW : v) & 0xff) << (8 * q);
        }
        *reinterpret_cast<unsigned*>(row + t0 + c) = packed;
    }
}

// =============================================================================================
// C ABI
// =============================================================================================
MMG_API int mmg_bootstrap_weights(unsigned long long seed, int n, int b0, int B, signed char* w, int ldw, hipStream_t stream) {
    const char* who = "mmg_bootstrap_weights";
    MMG_CHECK_ARG(w, "%s: null pointer", who);
    MMG_CHECK_ARG(n >= 1 && B >= 1 && b0 >= 0 && (long long)b0 + B <= 2147483647LL,
                  "%s: n and B must be positive and 0 <= b0, b0 + B < 2^31 (n=%d b0=%d B=%d)", who, n, b0, B);
    MMG_CHECK_ARG(B <= 65535, "%s: at most 65535 replicates per call (B=%d)", who, B);
    MMG_CHECK_ARG(ldw % 16 == 0 && ldw >= n, "%s: ldw must be a multiple of 16 and at least n padded to 16 (n=%d ldw=%d)", who, n, ldw);
    MMG_CHECK_ARG(((uintptr_t)w & 15) == 0, "%s: w must be 16-byte aligned", who);
    MMG_NOTE_KERNEL("bootstrap_weights_kernel");
    hipLaunchKernelGGL(bootstrap_weights_kernel, dim3(cdiv(ldw, BOOT_TILE), B), dim3(256), 0, stream,
                       mmg_drop_key(seed, SITE_BOOTSTRAP), n, b0, w, ldw);
    MMG_LAUNCH_CHECK(who);
    return 0;
}

MMG_API int mmg_auroc_pairs(const float* s_pos, const float* s_neg, const signed char* w_pos, int ldw_pos, const signed char* w_neg,
                            int ldw_neg, int P, int Nn, int B, long long* partial, hipStream_t stream) {
    const char* who = "mmg_auroc_pairs";
    MMG_CHECK_ARG(s_pos && s_neg && w_pos && w_neg && partial, "%s: null pointer", who);
    MMG_CHECK_ARG(P >= 1 && Nn >= 1 && B >= 1, "%s: P, Nn and B must be positive (P=%d Nn=%d B=%d)", who, P, Nn, B);
    MMG_CHECK_ARG(P <= 2147483647 - 32 && Nn <= 2147483647 - 64, "%s: P and Nn must leave room for the padding (P=%d Nn=%d)", who, P, Nn);
    MMG_CHECK_ARG(ldw_pos % 16 == 0 && ldw_pos >= P, "%s: ldw_pos must be a multiple of 16 and at least P padded to 16 (P=%d ldw_pos=%d)",
                  who, P, ldw_pos);
    MMG_CHECK_ARG(ldw_neg % 16 == 0 && ldw_neg >= Nn, "%s: ldw_neg must be a multiple of 16 and at least Nn padded to 16 (Nn=%d ldw_neg=%d)",
                  who, Nn, ldw_neg);
    MMG_CHECK_ARG(((uintptr_t)s_neg & 15) == 0 && ((uintptr_t)w_neg & 15) == 0, "%s: s_neg and w_neg must be 16-byte aligned", who);
    MMG_CHECK_ARG(cdiv(B, AUROC_COLS) <= 65535, "%s: too many replicates for one launch (B=%d)", who, B);
    MMG_NOTE_KERNEL("auroc_pairs_kernel");
    hipLaunchKernelGGL(auroc_pairs_kernel, dim3(cdiv(P, AUROC_ROWS), cdiv(B, AUROC_COLS)), dim3(AUROC_THREADS), 0, stream, s_pos, s_neg,
                       w_pos, ldw_pos, w_neg, ldw_neg, P, Nn, B, partial);
    MMG_LAUNCH_CHECK(who);
    return 0;
}
