// ConvNeXt stem in two launches: patch-embedding GEMM + LayerNorm, forward and backward (C = 96 / 128, kp = 32 / 64).
//
// The stem (torchvision ConvNeXt features[0]: Conv2d(Cin, C, 4, 4) -> LayerNorm2d; the reference runs it inside `model.features`,
// mmgclip/networks/encoder.py:53) has the tower's longest rows tensor - M = n (H/4) (W/4) rows - and a tiny matrix product (K = kp).
// The three-launch path (gemm_nt -> s0, layernorm_fwd; layernorm_bwd -> ds0, gemm_tn_acc) moves s0 and ds0, two [M,C] bf16 tensors that
// only carry a K = kp product between kernels, through HBM five times.  Here neither exists:
//   stem_fwd_kernel   reads p0 [M,kp], writes x = LN(bf16(p0 w^T + bias)) [M,C] (+ mean, rstd)
//   stem_bwd_kernel   reads dx [M,C], p0 and the statistics; recomputes s0, runs the LayerNorm backward in registers, rounds ds0 to bf16
//                     as the stored tensor was, and keeps dW = ds0^T p0, db = colsum(ds0), ln_dw, ln_db on chip for the whole launch
// Both round where the three-launch path stored bf16, so the results differ from it by fp32 summation order only.
//
// Work split: every WAVE is on its own - no workgroup barrier inside the row loops - and a workgroup is four of them; the grid is what is
// resident (CUs x workgroups per CU, fixed by __launch_bounds__), persistent over the rows.  Bytes in flight come from the waves per CU.
//
// Forward, per wave and 16 rows: the product is formed TRANSPOSED, D[channel][row] (A = w, B = p0^T: the B fragment of lane l is the
// 16 bytes p0[row l & 15][8 (l >> 4) ..], straight from global memory), so a lane holds 4 consecutive channels of ONE row per 16-channel
// tile: the row statistics are an in-lane sum plus two cross-lane steps, and the output leaves as 16-byte stores after one exchange of
// 8-byte pieces between lane pairs.  LDS holds gamma and beta only.
// Backward, per wave and 32 rows: D[row][channel] (A = p0, B = w^T), so that a lane holds ONE channel and 4 consecutive rows per tile
// and two 16-row tiles of ds0 ARE the A operand of dW += ds0^T p0 (k = the 32 rows; cnblock_bwdw.hip does the same).  dx and p0 go
// through a wave-private LDS image, written row-wise with 16-byte pieces and read back transposed (ds_read_b64_tr_b16): dx in the
// accumulator layout, p0 as the B operand with k = rows.  Row pitches of 2 C + 32 and 2 kp + 32 bytes make the transposed reads
// conflict-free.  Row sums of the LayerNorm backward run over the 16 lanes of a DPP row.
// Rows are addressed with 64-bit offsets (plain global loads / stores), so there is no 4 GiB buffer range to split a launch at.
#include "common.h"

typedef __attribute__((ext_vector_type(4))) unsigned st_u32x4;
typedef __attribute__((address_space(3))) bf16x4 st_lds_v4;

template <int C, int KP> struct StemCfg {
    static_assert((C == 96 || C == 128) && (KP == 32 || KP == 64), "stem: C in {96, 128}, kp in {32, 64}");
    static constexpr int CT = C / 16;              // 16-channel tiles
    static constexpr int KS = KP / 32;             // MFMA k-steps of the product
    static constexpr int NT = KP / 16;             // 16-column tiles of dW
    static constexpr int WAVES = 4;
    // backward LDS: [w fragments][per wave: p0 image, dx image, mean | rstd]; the end-of-launch reduction buffer aliases the images
    static constexpr int PP = KP * 2 + 32;         // p0 image row pitch (bytes)
    static constexpr int DP = C * 2 + 32;          // dx image row pitch
    static constexpr int RB = 32;                  // rows per backward step
    static constexpr int P0IMG = RB * PP, DXIMG = RB * DP, STIMG = 2 * RB * 4, WAVE_LDS = P0IMG + DXIMG + STIMG;
    static constexpr int WIMG = CT * KS * 1024;
    static constexpr int OFF_IMG = WIMG;
    static constexpr int RED = (C * KP + 3 * C) * 4;
    static constexpr int LDS = OFF_IMG + WAVES * WAVE_LDS;
    static_assert(RED <= WAVES * WAVE_LDS, "the reduction buffer aliases the row images");
    static_assert(LDS <= 80 * 1024, "two workgroups per CU");
    // waves per SIMD the backward's registers are budgeted for: dW alone is C kp / 64 accumulator registers per wave
    static constexpr int BWD_WPS = C * KP <= 96 * 32 ? 2 : 1;
};

struct StemFwdArgs {
    const bf16_t* p0; const bf16_t* w; const float* bias; const float* ln_w; const float* ln_b; float eps;
    bf16_t* x; float* mean; float* rstd; long long M; int nt;
};

struct StemBwdArgs {
    const bf16_t* dx; const bf16_t* p0; const bf16_t* w; const float* bias; const float* ln_w; const float* mean; const float* rstd;
    float* dW; float* db; float* ln_dw; float* ln_db; long long M;
};

__device__ __forceinline__ float st_sum16(float v) {       // sum over the 16 lanes of a DPP row
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xf, 0xf, true));   // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xf, 0xf, true));   // row_mirror
    return v;
}
__device__ __forceinline__ float st_sum_lg(float v) {      // sum over the 4 lanes {li, li + 16, li + 32, li + 48}
    v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ bf16x4 st_tr(const char* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((st_lds_v4*)p); }

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// WPS = waves per SIMD the register budget is set for (3: up to 168 registers; 2: 256)
template <int C, int KP, int WPS>
__global__ __launch_bounds__(256, WPS) void stem_fwd_kernel(const StemFwdArgs a) {
    typedef StemCfg<C, KP> Cfg;
    constexpr int CT = Cfg::CT, KS = Cfg::KS, G = 4;          // G 16-row groups = one 64-row tile per wave and iteration
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const bool odd = (lg & 1) != 0;

    // loaded once: w as A fragments (A[m = channel 16 ct + li][k = 32 ks + 8 lg + j]); bias, gamma, beta of this lane's channels 16 ct + 4 lg + e
    // (gamma and beta through LDS: 2 x CT x 4 registers less, which is what keeps C = 96 at three waves per SIMD)
    __shared__ __attribute__((aligned(16))) float s_gb[2 * C];
    for (int i = threadIdx.x; i < C; i += 256) { s_gb[i] = a.ln_w[i]; s_gb[C + i] = a.ln_b[i]; }
    __syncthreads();
    bf16x8 wf[CT][KS];
    f32x4 bia[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) wf[ct][ks] = *reinterpret_cast<const bf16x8*>(a.w + (size_t)(16 * ct + li) * KP + 32 * ks + 8 * lg);
        bia[ct] = *reinterpret_cast<const f32x4*>(a.bias + 16 * ct + 4 * lg);
    }
    const float inv_c = 1.0f / (float)C;
    const long long ntiles = (a.M + 63) / 64;
    for (long long t = (long long)blockIdx.x * Cfg::WAVES + wave; t < ntiles; t += (long long)gridDim.x * Cfg::WAVES) {
        const long long r0 = t * 64;
        // the tile's rows as B fragments (B[k][n = row li]); a row past the end reads the last row and stores nothing
        bf16x8 pf[G][KS];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const long long row = r0 + 16 * g + li, rc = row < a.M ? row : a.M - 1;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) pf[g][ks] = *reinterpret_cast<const bf16x8*>(a.p0 + (size_t)rc * KP + 32 * ks + 8 * lg);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const long long row = r0 + 16 * g + li;
            const bool live = row < a.M;
            f32x4 acc[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                acc[ct] = bia[ct];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ct][ks], pf[g][ks], acc[ct], 0, 0, 0);
            }
            // s0 = bf16(product + bias), as the three-launch path stored it; LayerNorm over the row's C channels (4 lanes x CT x 4)
            float s = 0.f;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc[ct][e] = bf2f(f2bf(acc[ct][e])); s += acc[ct][e]; }
            const float mu = st_sum_lg(s) * inv_c;
            float q = 0.f;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc[ct][e] -= mu; q += acc[ct][e] * acc[ct][e]; }
            const float rs = rsqrtf(st_sum_lg(q) * inv_c + a.eps);
            unsigned pk[CT][2];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const f32x4 gam = *reinterpret_cast<const f32x4*>(s_gb + 16 * ct + 4 * lg), bet = *reinterpret_cast<const f32x4*>(s_gb + C + 16 * ct + 4 * lg);
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = acc[ct][e] * rs * gam[e] + bet[e];
                pk[ct][0] = pack2bf(o[0], o[1]); pk[ct][1] = pack2bf(o[2], o[3]);
            }
            // 8-byte pieces -> 16-byte stores: lanes lg and lg ^ 1 exchange one piece per pair of channel tiles; the even lane then
            // holds channels 32 c + 4 lg .. + 7, the odd one 32 c + 16 + 4 (lg - 1) .. + 7
            bf16_t* xrow = a.x + (size_t)(live ? row : 0) * C;
#pragma unroll
            for (int c = 0; c < CT / 2; ++c) {
                const unsigned s0 = odd ? pk[2 * c][0] : pk[2 * c + 1][0], s1 = odd ? pk[2 * c][1] : pk[2 * c + 1][1];
                const unsigned r0_ = __shfl_xor(s0, 16, 64), r1_ = __shfl_xor(s1, 16, 64);
                const uint4 v = odd ? make_uint4(r0_, r1_, pk[2 * c + 1][0], pk[2 * c + 1][1]) : make_uint4(pk[2 * c][0], pk[2 * c][1], r0_, r1_);
                const int ch = odd ? 32 * c + 16 + 4 * (lg - 1) : 32 * c + 4 * lg;
                if (live) store16_stream(xrow + ch, v, a.nt != 0);
            }
            if (live && lg == 0) {
                if (a.mean) a.mean[row] = mu;
                if (a.rstd) a.rstd[row] = rs;
            }
            __builtin_amdgcn_sched_barrier(0);          // one group after the other: interleaved, their temporaries do not fit the register budget
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
template <int C, int KP>
__global__ __launch_bounds__(256, (StemCfg<C, KP>::BWD_WPS)) void stem_bwd_kernel(const StemBwdArgs a) {
    typedef StemCfg<C, KP> Cfg;
    constexpr int CT = Cfg::CT, KS = Cfg::KS, NT = Cfg::NT, PP = Cfg::PP, DP = Cfg::DP, RB = Cfg::RB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;

    // w as B fragments (B[k = 32 ks + 8 lg + j][n = channel 16 ct + li]) in LDS, [ct][ks][lane] x 16 bytes: read lane-linear every step
    for (int i = tid; i < CT * KS * 64; i += 256) {
        const int l = i & 63, ks = (i >> 6) % KS, ct = (i >> 6) / KS;
        *reinterpret_cast<uint4*>(smem + i * 16) = *reinterpret_cast<const uint4*>(a.w + (size_t)(16 * ct + (l & 15)) * KP + 32 * ks + 8 * (l >> 4));
    }
    float gam[CT], bia[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) { gam[ct] = a.ln_w[16 * ct + li]; bia[ct] = a.bias[16 * ct + li]; }
    __syncthreads();

    char* pimg = smem + Cfg::OFF_IMG + wave * Cfg::WAVE_LDS;       // this wave's images: p0 [32][PP], dx [32][DP]
    char* dimg = pimg + Cfg::P0IMG;
    float* simg = reinterpret_cast<float*>(dimg + Cfg::DXIMG);   // [mean of 32 rows][rstd of 32 rows]
    const int p_wr = li * PP + lg * 16;                            // + t2 * 16 PP + ks * 64
    const int tr_p = (4 * lg + q) * PP + 8 * p;                    // + t2 * 16 PP + nt * 32
    const int tr_d = (4 * lg + q) * DP + 8 * p;                    // + t2 * 16 DP + ct * 32

    f32x4 dwacc[CT][NT];                                           // dW[channel 16 ct + 4 lg + e][k 16 nt + li]
    float dg[CT], dbt[CT], dbs[CT];                                // ln_dw, ln_db, db of channel 16 ct + li
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        dg[ct] = 0.f; dbt[ct] = 0.f; dbs[ct] = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) dwacc[ct][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float inv_c = 1.0f / (float)C;
    const long long nsteps = (a.M + RB - 1) / RB;
    for (long long st = (long long)blockIdx.x * Cfg::WAVES + wave; st < nsteps; st += (long long)gridDim.x * Cfg::WAVES) {
        const long long r0 = st * RB;
        // ---- global loads: p0 rows as A fragments (A[m = row li][k]), dx rows in 16-byte pieces, one statistic per lane.
        // A row past the end reads the last row; its dx is replaced by zero, so its ds0 is zero and it adds nothing anywhere.
        bf16x8 pa[2][KS];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            const long long row = r0 + 16 * t2 + li, rc = row < a.M ? row : a.M - 1;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) pa[t2][ks] = *reinterpret_cast<const bf16x8*>(a.p0 + (size_t)rc * KP + 32 * ks + 8 * lg);
        }
        uint4 dxr[CT];                                             // 32 rows x 2 C bytes = CT x 64 lanes x 16 bytes
        int d_wr[CT];
#pragma unroll
        for (int n = 0; n < CT; ++n) {
            const int byte = (lane + 64 * n) * 16, r = byte / (2 * C), cb = byte % (2 * C);
            const long long row = r0 + r;
            const bool live = row < a.M;
            const uint4 v = *reinterpret_cast<const uint4*>(a.dx + (size_t)(live ? row : a.M - 1) * C + cb / 2);
            dxr[n] = live ? v : make_uint4(0u, 0u, 0u, 0u);
            d_wr[n] = r * DP + cb;
        }
        float stat;                                                // lanes 0 - 31: mean of row r0 + lane; 32 - 63: rstd of row r0 + lane - 32
        {
            const long long row = r0 + (lane & 31), rc = row < a.M ? row : a.M - 1;
            stat = lane < 32 ? a.mean[rc] : a.rstd[rc];
        }
        // ---- the wave's LDS images.  LDS executes one wave's instructions in order, so the previous step's reads are done before
        // these writes and the reads below see them; the two asm statements keep the compiler from moving either across.
        asm volatile("" ::: "memory");
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) *reinterpret_cast<bf16x8*>(pimg + p_wr + t2 * 16 * PP + ks * 64) = pa[t2][ks];
#pragma unroll
        for (int n = 0; n < CT; ++n) *reinterpret_cast<uint4*>(dimg + d_wr[n]) = dxr[n];
        simg[lane] = stat;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

        // ---- s0, LayerNorm backward, ds0 (bf16) as the A operand of the weight-gradient product: one 16-row tile after the other
        unsigned dsu[CT][4];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            float xh[CT][4];
            bf16x4 dq[CT];
            const f32x4 mu = *reinterpret_cast<const f32x4*>(simg + 16 * t2 + 4 * lg), rs = *reinterpret_cast<const f32x4*>(simg + RB + 16 * t2 + 4 * lg);
            float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa[t2][ks], *reinterpret_cast<const bf16x8*>(smem + ((ct * KS + ks) * 64 + lane) * 16), acc, 0, 0, 0);
                dq[ct] = st_tr(dimg + tr_d + t2 * 16 * DP + ct * 32);                   // dx[row 16 t2 + 4 lg + e][channel 16 ct + li]
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float s0 = bf2f(f2bf(acc[e] + bia[ct]));
                    const float x = (s0 - mu[e]) * rs[e], dv = bf2f((bf16_t)dq[ct][e]), g = dv * gam[ct];
                    xh[ct][e] = x;
                    s1[e] += g;
                    s2[e] += g * x;
                    dg[ct] += dv * x;
                    dbt[ct] += dv;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { s1[e] = st_sum16(s1[e]) * inv_c; s2[e] = st_sum16(s2[e]) * inv_c; }
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = rs[e] * (bf2f((bf16_t)dq[ct][e]) * gam[ct] - s1[e] - xh[ct][e] * s2[e]);
                    dbs[ct] += bf2f(f2bf(o[e]));
                }
                dsu[ct][2 * t2] = pack2bf(o[0], o[1]); dsu[ct][2 * t2 + 1] = pack2bf(o[2], o[3]);
            }
        }
        // ---- dW += ds0^T p0: k = the 32 rows (slot 8 lg + j: j < 4 row 4 lg + j, else row 16 + 4 lg + j - 4), p0 by transposed reads
        bf16x8 pt[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const bf16x4 lo = st_tr(pimg + tr_p + nt * 32), hi = st_tr(pimg + tr_p + 16 * PP + nt * 32);
            pt[nt] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const bf16x8 df = __builtin_bit_cast(bf16x8, (st_u32x4{dsu[ct][0], dsu[ct][1], dsu[ct][2], dsu[ct][3]}));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) dwacc[ct][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, pt[nt], dwacc[ct][nt], 0, 0, 0);
        }
    }

    // ---- the accumulators leave: four waves summed in LDS (over the row images), then one fp32 atomic per element and workgroup
    float* red = reinterpret_cast<float*>(smem + Cfg::OFF_IMG);
    __syncthreads();
    for (int i = tid; i < C * KP + 3 * C; i += 256) red[i] = 0.f;
    __syncthreads();
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int e = 0; e < 4; ++e) atomicAdd(&red[(16 * ct + 4 * lg + e) * KP + 16 * nt + li], dwacc[ct][nt][e]);
        const float g = st_sum_lg(dg[ct]), b = st_sum_lg(dbt[ct]), s = st_sum_lg(dbs[ct]);
        if (lg == 0) {
            atomicAdd(&red[C * KP + 16 * ct + li], g);
            atomicAdd(&red[C * KP + C + 16 * ct + li], b);
            atomicAdd(&red[C * KP + 2 * C + 16 * ct + li], s);
        }
    }
    __syncthreads();
    for (int i = tid; i < C * KP; i += 256) atomicAdd(a.dW + i, red[i]);
    for (int i = tid; i < C; i += 256) {
        atomicAdd(a.ln_dw + i, red[C * KP + i]);
        atomicAdd(a.ln_db + i, red[C * KP + C + i]);
        atomicAdd(a.db + i, red[C * KP + 2 * C + i]);
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------------
MMG_API int mmg_stem_supported(int C, int kp) { return (C == 96 || C == 128) && (kp == 32 || kp == 64) ? 1 : 0; }

template <int C, int KP, int WPS>
static void stem_fwd_launch(const StemFwdArgs& a, hipStream_t stream) {
    const long long wg_tiles = (a.M + 255) / 256;                 // 4 waves x 64 rows
    const long long cap = (long long)mmg_cu_count_cached() * WPS; // resident: WPS workgroups of 4 waves per CU
    hipLaunchKernelGGL((stem_fwd_kernel<C, KP, WPS>), dim3((unsigned)(wg_tiles < cap ? wg_tiles : cap)), dim3(256), 0, stream, a);
}

template <int C, int KP>
static void stem_bwd_launch(const StemBwdArgs& a, hipStream_t stream) {
    typedef StemCfg<C, KP> Cfg;
    const long long wg_steps = (a.M + 4 * Cfg::RB - 1) / (4 * Cfg::RB);
    const long long cap = (long long)mmg_cu_count_cached() * Cfg::BWD_WPS;
    mmg_allow_lds(stem_bwd_kernel<C, KP>, Cfg::LDS);
    hipLaunchKernelGGL((stem_bwd_kernel<C, KP>), dim3((unsigned)(wg_steps < cap ? wg_steps : cap)), dim3(256), Cfg::LDS, stream, a);
}

MMG_API int mmg_stem_fwd(const void* p0, const void* w, const float* bias, const float* ln_w, const float* ln_b, float eps, void* x,
                         float* mean, float* rstd, long long M, int C, int kp, hipStream_t stream) {
    MMG_CHECK_ARG(mmg_stem_supported(C, kp), "mmg_stem_fwd: C=%d kp=%d is not supported (C in {96, 128}, kp in {32, 64})", C, kp);
    MMG_CHECK_ARG(M > 0, "mmg_stem_fwd: M=%lld must be positive", M);
    MMG_CHECK_ARG(p0 && w && bias && ln_w && ln_b && x, "mmg_stem_fwd: null pointer");
    MMG_CHECK_ARG((mean == nullptr) == (rstd == nullptr), "mmg_stem_fwd: mean and rstd are saved together (both or neither)");
    StemFwdArgs a{(const bf16_t*)p0, (const bf16_t*)w, bias, ln_w, ln_b, eps, (bf16_t*)x, mean, rstd, M,
                  M * C * 2 >= (256LL << 20) ? 1 : 0};           // streaming stores for an output the Infinity Cache cannot hold
    MMG_NOTE_KERNEL("stem_fwd_kernel<%d, %d, %d>", C, kp, C == 96 && kp == 32 ? 3 : 2);      // (as the branches below instantiate it)
    if (C == 96 && kp == 32) stem_fwd_launch<96, 32, 3>(a, stream);
    else if (C == 96) stem_fwd_launch<96, 64, 2>(a, stream);
    else if (kp == 32) stem_fwd_launch<128, 32, 2>(a, stream);
    else stem_fwd_launch<128, 64, 2>(a, stream);
    MMG_LAUNCH_CHECK("mmg_stem_fwd");
    return 0;
}

MMG_API int mmg_stem_bwd(const void* dx, const void* p0, const void* w, const float* bias, const float* ln_w, const float* mean,
                         const float* rstd, float* dW, float* db, float* ln_dw, float* ln_db, long long M, int C, int kp,
                         hipStream_t stream) {
    MMG_CHECK_ARG(mmg_stem_supported(C, kp), "mmg_stem_bwd: C=%d kp=%d is not supported (C in {96, 128}, kp in {32, 64})", C, kp);
    MMG_CHECK_ARG(M > 0, "mmg_stem_bwd: M=%lld must be positive", M);
    MMG_CHECK_ARG(dx && p0 && w && bias && ln_w && mean && rstd && dW && db && ln_dw && ln_db, "mmg_stem_bwd: null pointer");
    StemBwdArgs a{(const bf16_t*)dx, (const bf16_t*)p0, (const bf16_t*)w, bias, ln_w, mean, rstd, dW, db, ln_dw, ln_db, M};
    MMG_NOTE_KERNEL("stem_bwd_kernel<%d, %d>", C, kp);
    if (C == 96 && kp == 32) stem_bwd_launch<96, 32>(a, stream);
    else if (C == 96) stem_bwd_launch<96, 64>(a, stream);
    else if (kp == 32) stem_bwd_launch<128, 32>(a, stream);
    else stem_bwd_launch<128, 64>(a, stream);
    MMG_LAUNCH_CHECK("mmg_stem_bwd");
    return 0;
}
