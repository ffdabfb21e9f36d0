// Data-gradient GEMM with the LayerNorm backward in its epilogue (gfx950): dx = LNbwd(bf16(A B^T), x) in one launch.
//
// In the ConvNeXt backward (mmgclip/networks/convnext.py) an NT GEMM whose only reader is a LayerNorm backward sits in front of every
// stage-3 block's LayerNorm (dln = dh W1) and of every downsample layer's (dld = dx Wt, 2x2-patchified).  The pair moves four [M,N]
// streams: the GEMM writes dln, layernorm_bwd_plain_kernel reads it and x and writes dx.  Here dln stays on chip: x is read, dx written.
//   dln = bf16(A[M,K] B[N,K]^T)                    fp32 accumulation, rounded as the stored tensor was
//   per pixel (C consecutive columns of a row):    xhat = (x - mean) rstd,  g = dln gamma,
//       dx = bf16(rstd (g - mean_C(g) - xhat mean_C(g xhat))),  dgamma += sum dln xhat,  dbeta += sum dln
// patch = 0: N = C, GEMM row r is LayerNorm row r.  patch = 1: N = 4C, GEMM row r = (n, ph, pw) and segment s of it are pixel
// (n, 2 ph + s / 2, 2 pw + s % 2) of an H x W map (the inverse of ln_out_offset, norm_elementwise.hip); x, dx, mean, rstd by pixel.
//
// Tile 128 x 384 x 64, 8 waves as 2 (M) x 4 (N), wave tile 64 x 96: 384 columns hold whole pixels at C = 96 / 192 / 384.  The main loop is
// gemm_nt_kernel's (gemm_bf16.hip): 16-byte LDS-DMA staging with the swizzle on the source address, per-thread constant offsets, two stages
// of 64 KB, the MFMA issued swapped so a lane holds 4 consecutive columns of a row.
// Epilogue: dln is EXACTLY a bf16 value, so the accumulators cross LDS packed to bf16 - the whole 128 x 384 tile (98 KB) fits over the stages at once
// where an fp32 image would need two 64-row slabs, every wave's 96 accumulator registers are free before the LayerNorm arithmetic starts, and the
// row pass reads half the LDS bytes.  The row pass is layernorm_bwd_plain_kernel's, lane for lane: a pixel is owned by G = C / 24 lanes with 3
// chunks of 8 columns each (chunk = lane + k G), the sums run over group_sum's DPP butterfly (G <= 16: no cross-row step), so dx has the bits the
// pair gives.  A wave covers 4 tile rows per pass, the workgroup 32, four passes.
// x, mean and rstd of the first pass (3 x 16 bytes + 2 floats per lane, from clamped addresses, unconditionally) are requested BEFORE the main
// loop - their latency is under the K tiles -, those of the other three behind it, under the image's barriers and the first pass (the registers
// of all four would not fit beside the accumulators and the column sums).
// The grid is persistent: one workgroup per CU walks a contiguous run of tiles (column tiles of one row panel follow each other: the A panel is in L2),
// and dgamma / dbeta stay in registers for the whole run - one LDS reduction and one set of global fp32 atomics per WORKGROUP, as
// layernorm_bwd_plain_kernel has it (per tile it would be 32 768 x 192 same-line atomics at the first downsample layer).
// Rows past M are loaded from clamped addresses, count as dln = 0 and are never stored.  x and dx rows use 64-bit offsets.
#include "common.h"

#define LNB_BM 128
#define LNB_BN 384
#define LNB_BK 64
#define LNB_THREADS 512
#define LNB_STAGE ((LNB_BM + LNB_BN) * LNB_BK * 2)          // 64 KB
#define LNB_PITCH (LNB_BN * 2 + 16)                         // bytes per row of the bf16 tile image (16-byte aligned; 196 words: rows 4 banks apart)
#define LNB_RED (2 * LNB_STAGE)                             // [2][384] floats behind the stages (lives for the whole launch)
#define LNB_GAM (LNB_RED + 2 * LNB_BN * 4)                  // gamma [384] floats behind that
#define LNB_LDS (LNB_GAM + LNB_BN * 4)
static_assert(LNB_BM * LNB_PITCH <= 2 * LNB_STAGE, "the tile image aliases the two stages");
static_assert(LNB_LDS <= 160 * 1024, "LDS of a CU");

struct GemmLnBwd {
    const bf16_t* A; const bf16_t* B;
    int M, N, K, lda, ldb;
    const bf16_t* x; int ldx;
    const float* mean; const float* rstd; const float* gamma;
    bf16_t* dx; int lddx;
    float* dgamma; float* dbeta;
    int H, W;
    int tiles_n, tiles;
    int nt;
};

__device__ __forceinline__ void lnb_glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// sum over the G <= 16 lanes of a group, inside one DPP row (norm_elementwise.hip: group_sum)
template <int G>
__device__ __forceinline__ float lnb_group_sum(float v) {
    if (G >= 2) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
    if (G >= 4) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
    if (G >= 8) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xf, 0xf, true));   // row_half_mirror
    if (G >= 16) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xf, 0xf, true));  // row_mirror
    return v;
}

__device__ __forceinline__ void lnb_unpack8(const uint4 v, float* f) {
    f[0] = bf2f_lo(v.x); f[1] = bf2f_hi(v.x); f[2] = bf2f_lo(v.y); f[3] = bf2f_hi(v.y);
    f[4] = bf2f_lo(v.z); f[5] = bf2f_hi(v.z); f[6] = bf2f_lo(v.w); f[7] = bf2f_hi(v.w);
}

template <int C, int PATCH>
__global__ __launch_bounds__(LNB_THREADS, 1) void gemm_nt_lnbwd_kernel(const GemmLnBwd g) {
    static_assert(C == 96 || C == 192 || C == 384, "a 384-column tile holds whole pixels");
    static_assert(PATCH == 1 || C == LNB_BN, "plain rows: N = C = one column tile");
    constexpr int BM = LNB_BM, BN = LNB_BN, BK = LNB_BK, THREADS = LNB_THREADS;
    constexpr int MI = 4, NI = 6;                         // 16 x 16 fragments per wave (wave tile 64 x 96)
    constexpr int A_BYTES = BM * BK * 2, STAGE = LNB_STAGE;
    constexpr int CPR = BK / 8;                           // 16-byte chunks per staged row
    constexpr int A_IT = BM * CPR / THREADS, B_IT = BN * CPR / THREADS;      // 2, 6
    constexpr int G = C / 24, CH = 3;                     // lanes per pixel, 8-column chunks per lane
    constexpr int SEG = BN / C;                           // pixels per tile row
    constexpr int PASSES = BM / 32;                       // a wave covers 4 tile rows per pass
    constexpr int PRE = 1, POST = PASSES - PRE;           // passes whose reads are requested before / behind the main loop
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 2, wn = wave & 3;
    const int li = lane & 15, lg = lane >> 4;
    const int gi = lane / G, gl = lane % G;               // pixel of this wave's pass, lane inside the pixel
    const int prow = wave * 4 + gi / SEG, seg = gi % SEG; // tile row (+ 32 per pass), pixel inside the row

    float* red = reinterpret_cast<float*>(smem + LNB_RED);         // [2][C], behind the stages
    float* sgam = reinterpret_cast<float*>(smem + LNB_GAM);
    for (int i = tid; i < 2 * C; i += THREADS) red[i] = 0.f;       // (ordered before their use by every barrier of the tile loop)
    for (int i = tid; i < C; i += THREADS) sgam[i] = g.gamma[i];

    // ---- per-thread constants of the staging and of the fragment reads ------------------------------------------------------------------
    // (N % 384 == 0: every B row of the tile exists; pass `it` of the B staging is 64 rows further down - a uniform step, r & 7 unchanged)
    const unsigned b_off = (unsigned)((tid / CPR) * g.ldb + ((tid % CPR) ^ ((tid / CPR) & 7)) * 8) * 2u;
    const size_t b_step = (size_t)(THREADS / CPR) * g.ldb * 2;
    char* lds_wave = smem + (tid & ~63) * 16;                              // wave-uniform LDS-DMA base
    int a_frag[BK / 32], b_frag[BK / 32];
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
        const int ra = wm * 64 + li, rb = wn * 96 + li;                    // rows of fragment 0; fragment i adds 16 rows (same r & 7)
        a_frag[ks] = ra * (BK * 2) + (((4 * ks + lg) ^ (ra & 7)) << 4);
        b_frag[ks] = A_BYTES + rb * (BK * 2) + (((4 * ks + lg) ^ (rb & 7)) << 4);
    }
    const int nk = g.K / BK;
    const float inv_c = 1.0f / (float)C;

    float dg[CH][8], db[CH][8];                                            // this lane's 24 columns, over every row of every tile
#pragma unroll
    for (int k = 0; k < CH; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) { dg[k][e] = 0.f; db[k][e] = 0.f; }

    const int t_begin = (int)((long long)blockIdx.x * g.tiles / gridDim.x), t_end = (int)((long long)(blockIdx.x + 1) * g.tiles / gridDim.x);
    for (int t = t_begin; t < t_end; ++t) {
        const int tm = t / g.tiles_n, tn = t - tm * g.tiles_n;
        const int m0 = tm * BM, n0 = tn * BN;
        const int s = n0 / C + seg;                                        // segment of the GEMM row (patch: the 2 x 2 position)

        unsigned a_off[A_IT];                                              // global byte offsets inside the tile, rows clamped
#pragma unroll
        for (int it = 0; it < A_IT; ++it) {
            const int p = it * THREADS + tid, r = p / CPR, sl = p % CPR;
            const int gr = min(m0 + r, g.M - 1) - m0;
            a_off[it] = (unsigned)(gr * g.lda + (sl ^ (r & 7)) * 8) * 2u;
        }
        const char* a_base = reinterpret_cast<const char*>(g.A + (size_t)m0 * g.lda);   // uniform; advanced by BK per K tile
        const char* b_base = reinterpret_cast<const char*>(g.B + (size_t)n0 * g.ldb);
        auto stage = [&](int buf, int kt) {
            const char* ab = a_base + (size_t)kt * (BK * 2);
            const char* bb = b_base + (size_t)kt * (BK * 2);
            char* la = lds_wave + buf * STAGE;
#pragma unroll
            for (int it = 0; it < A_IT; ++it) lnb_glds16(ab + a_off[it], la + it * THREADS * 16);
#pragma unroll
            for (int it = 0; it < B_IT; ++it) lnb_glds16(bb + it * b_step + b_off, la + A_BYTES + it * THREADS * 16);
        };
        // (the previous tile's image is dead: the barrier that ends its row pass is behind every wave)
        stage(0, 0);

        // ---- the row pass's global reads: clamped addresses, unconditional; a row past M is loaded and never stored ------------------
        int pix[PASSES];                                                   // (the launch checks that the pixels fit an int)
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int r = min(m0 + p * 32 + prow, g.M - 1);
            if constexpr (PATCH) {
                const int w2 = g.W >> 1, h2 = g.H >> 1;
                const int pw = r % w2, ph = (r / w2) % h2, n = r / (w2 * h2);
                pix[p] = (n * g.H + 2 * ph + (s >> 1)) * g.W + 2 * pw + (s & 1);
            } else {
                pix[p] = r;
            }
        }
        uint4 xa[PRE][CH], xb[POST][CH];
        float mua[PRE], rsa[PRE], mub[POST], rsb[POST];
#pragma unroll
        for (int p = 0; p < PRE; ++p) {
#pragma unroll
            for (int k = 0; k < CH; ++k) xa[p][k] = *reinterpret_cast<const uint4*>(g.x + (size_t)pix[p] * g.ldx + (gl + k * G) * 8);
            mua[p] = g.mean[pix[p]];
            rsa[p] = g.rstd[pix[p]];
        }

        f32x4 acc[MI][NI];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int kt0 = 0; kt0 < nk; kt0 += 2) {
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
                const int kt = kt0 + sb;
                if (kt < nk) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                    if (kt + 1 < nk) stage(sb ^ 1, kt + 1);
                    const char* buf = smem + sb * STAGE;
#pragma unroll
                    for (int ks = 0; ks < BK / 32; ++ks) {
                        bf16x8 af[MI], bfr[NI];
#pragma unroll
                        for (int i = 0; i < MI; ++i) af[i] = *reinterpret_cast<const bf16x8*>(buf + a_frag[ks] + i * 16 * BK * 2);
#pragma unroll
                        for (int j = 0; j < NI; ++j) bfr[j] = *reinterpret_cast<const bf16x8*>(buf + b_frag[ks] + j * 16 * BK * 2);
#pragma unroll
                        for (int i = 0; i < MI; ++i)
#pragma unroll
                            for (int j = 0; j < NI; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
                    }
                }
            }
        }

        // ---- accumulators -> bf16 tile image over the stages.  LDS ordering is all these barriers need (gemm_bf16.hip): a __syncthreads() would
        // also wait for every global access in flight (on CDNA4 vmcnt counts stores too): the reads requested between them, later tiles' pending dx stores
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");    // every wave's fragment reads are done
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
                *reinterpret_cast<uint2*>(smem + (wm * 64 + i * 16 + li) * LNB_PITCH + (wn * 96 + j * 16 + 4 * lg) * 2) =
                    make_uint2(pack2bf(acc[i][j][0], acc[i][j][1]), pack2bf(acc[i][j][2], acc[i][j][3]));
        __builtin_amdgcn_sched_barrier(0);      // (the reads below are requested once the accumulators are dead)
#pragma unroll
        for (int p = 0; p < POST; ++p) {
#pragma unroll
            for (int k = 0; k < CH; ++k) xb[p][k] = *reinterpret_cast<const uint4*>(g.x + (size_t)pix[PRE + p] * g.ldx + (gl + k * G) * 8);
            mub[p] = g.mean[pix[PRE + p]];
            rsb[p] = g.rstd[pix[PRE + p]];
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

        // ---- the LayerNorm backward of the tile's pixels (layernorm_bwd_plain_kernel's arithmetic, lane for lane) -----------------------
        float gam[CH][8];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int c = gl + k * G;
            const float4 g0 = *reinterpret_cast<const float4*>(sgam + c * 8), g1 = *reinterpret_cast<const float4*>(sgam + c * 8 + 4);
            gam[k][0] = g0.x; gam[k][1] = g0.y; gam[k][2] = g0.z; gam[k][3] = g0.w; gam[k][4] = g1.x; gam[k][5] = g1.y; gam[k][6] = g1.z; gam[k][7] = g1.w;
        }
        auto row_pass = [&](int p, const uint4* xr, float mu, float rs) {
            const int rl = p * 32 + prow;
            const bool live = m0 + rl < g.M;
            uint4 dr[CH];
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                dr[k] = *reinterpret_cast<const uint4*>(smem + rl * LNB_PITCH + (seg * C + (gl + k * G) * 8) * 2);
                if (!live) dr[k] = make_uint4(0u, 0u, 0u, 0u);
            }
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                float xv[8], dyv[8];
                lnb_unpack8(xr[k], xv);
                lnb_unpack8(dr[k], dyv);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xh = (xv[e] - mu) * rs, gg = dyv[e] * gam[k][e];
                    s1 += gg;
                    s2 += gg * xh;
                    dg[k][e] += dyv[e] * xh;
                    db[k][e] += dyv[e];
                }
            }
            // the column sums take this pass's terms NOW: hipcc otherwise keeps the 48 products of every pass to the end of the tile and adds
            // them there as packed pairs, with dg / db spilled around the main loop to make room
#pragma unroll
            for (int k = 0; k < CH; ++k)
#pragma unroll
                for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(dg[k][e]), "+v"(db[k][e]));
            s1 = lnb_group_sum<G>(s1) * inv_c;
            s2 = lnb_group_sum<G>(s2) * inv_c;
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                float xv[8], dyv[8], o[8];
                lnb_unpack8(xr[k], xv);
                lnb_unpack8(dr[k], dyv);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = rs * (dyv[e] * gam[k][e] - s1 - (xv[e] - mu) * rs * s2);
                if (live)
                    store16_stream(g.dx + (size_t)pix[p] * g.lddx + (gl + k * G) * 8,
                                   make_uint4(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]), pack2bf(o[4], o[5]), pack2bf(o[6], o[7])), g.nt != 0);
            }
        };
#pragma unroll
        for (int p = 0; p < PRE; ++p) row_pass(p, xa[p], mua[p], rsa[p]);
#pragma unroll
        for (int p = 0; p < POST; ++p) row_pass(PRE + p, xb[p], mub[p], rsb[p]);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");    // the image is read: the next tile may stage over it
    }

    if (g.dgamma) {
#pragma unroll
        for (int k = 0; k < CH; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                atomicAdd(&red[(gl + k * G) * 8 + e], dg[k][e]);
                atomicAdd(&red[C + (gl + k * G) * 8 + e], db[k][e]);
            }
        __syncthreads();
        for (int i = tid; i < C; i += THREADS) {
            atomicAdd(g.dgamma + i, red[i]);
            atomicAdd(g.dbeta + i, red[C + i]);
        }
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------------
static const char* lnb_shape_error(int N, int K, int C, int patch, int H, int W) {
    if (!(C == 96 || C == 192 || C == 384)) return "C must be 96, 192 or 384";
    if (!(patch == 0 || patch == 1)) return "patch must be 0 or 1";
    if (N <= 0 || N % LNB_BN != 0) return "N must be a positive multiple of 384";
    if (K < LNB_BK || K % LNB_BK != 0) return "K must be a positive multiple of 64";
    if (patch == 0 && N != C) return "plain rows need N == C";
    if (patch == 1 && N != 4 * C) return "patchified rows need N == 4 C";
    if (patch == 1 && (H < 2 || W < 2 || (H & 1) || (W & 1))) return "patchified rows need even H and W (odd maps: the two-launch path)";
    return nullptr;
}

MMG_API int mmg_gemm_nt_lnbwd_supported(int N, int K, int C, int patch, int H, int W) {
    return lnb_shape_error(N, K, C, patch, H, W) == nullptr ? 1 : 0;
}

template <int C, int PATCH>
static void lnb_launch(const GemmLnBwd& g, hipStream_t stream) {
    const int cus = mmg_cu_count_cached();                         // persistent: one workgroup (128 KB of LDS) per CU
    mmg_allow_lds(gemm_nt_lnbwd_kernel<C, PATCH>, LNB_LDS);
    MMG_NOTE_KERNEL("gemm_nt_lnbwd_kernel<%d, %d>", C, PATCH);
    hipLaunchKernelGGL((gemm_nt_lnbwd_kernel<C, PATCH>), dim3(g.tiles < cus ? g.tiles : cus), dim3(LNB_THREADS), LNB_LDS, stream, g);
}

MMG_API int mmg_gemm_nt_lnbwd(const void* A, int lda, const void* B, int ldb, int M, int N, int K, const void* x, int ldx,
                              const float* mean, const float* rstd, const float* gamma, void* dx, int lddx, float* dgamma, float* dbeta,
                              int C, int patch, int H, int W, hipStream_t stream) {
    const char* why = lnb_shape_error(N, K, C, patch, H, W);
    MMG_CHECK_ARG(why == nullptr, "mmg_gemm_nt_lnbwd: N=%d K=%d C=%d patch=%d H=%d W=%d is not supported: %s", N, K, C, patch, H, W, why ? why : "");
    MMG_CHECK_ARG(M >= 1, "mmg_gemm_nt_lnbwd: M=%d must be positive", M);
    MMG_CHECK_ARG(patch == 0 || M % ((H / 2) * (W / 2)) == 0,
                  "mmg_gemm_nt_lnbwd: M=%d is not supported: not a multiple of the (H/2)(W/2) = %d patch rows of an image", M, (H / 2) * (W / 2));
    MMG_CHECK_ARG((long long)M * (patch ? 4 : 1) <= 0x7fffffffLL, "mmg_gemm_nt_lnbwd: M=%d has too many pixels", M);
    MMG_CHECK_ARG(lda >= K && ldb >= K && ldx >= C && lddx >= C, "mmg_gemm_nt_lnbwd: a leading dimension is shorter than its row (lda=%d ldb=%d K=%d ldx=%d lddx=%d C=%d)",
                  lda, ldb, K, ldx, lddx, C);
    MMG_CHECK_ARG(lda % 8 == 0 && ldb % 8 == 0 && ldx % 8 == 0 && lddx % 8 == 0, "mmg_gemm_nt_lnbwd: leading dimensions must be multiples of 8 (16-byte rows)");
    MMG_CHECK_ARG((long long)LNB_BM * lda * 2 <= 0x7fffffffLL && (long long)LNB_BN * ldb * 2 <= 0x7fffffffLL, "mmg_gemm_nt_lnbwd: lda=%d / ldb=%d too large", lda, ldb);
    MMG_CHECK_ARG(A && B && x && mean && rstd && gamma && dx, "mmg_gemm_nt_lnbwd: null pointer");
    MMG_CHECK_ARG((dgamma == nullptr) == (dbeta == nullptr), "mmg_gemm_nt_lnbwd: dgamma and dbeta are accumulated together (both or neither)");
    MMG_CHECK_ARG((((uintptr_t)A | (uintptr_t)B | (uintptr_t)x | (uintptr_t)dx) & 15) == 0, "mmg_gemm_nt_lnbwd: A, B, x and dx must be 16-byte aligned");
    const long long tiles = (long long)cdiv(M, LNB_BM) * (N / LNB_BN);
    MMG_CHECK_ARG(tiles <= 0x7fffffffLL, "mmg_gemm_nt_lnbwd: too many tiles");
    GemmLnBwd g;
    g.A = (const bf16_t*)A; g.B = (const bf16_t*)B; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb;
    g.x = (const bf16_t*)x; g.ldx = ldx; g.mean = mean; g.rstd = rstd; g.gamma = gamma; g.dx = (bf16_t*)dx; g.lddx = lddx;
    g.dgamma = dgamma; g.dbeta = dbeta; g.H = H; g.W = W;
    g.tiles_n = N / LNB_BN; g.tiles = (int)tiles;
    g.nt = (size_t)M * N * 2 >= ((size_t)256 << 20) ? 1 : 0;       // streaming stores for a dx the Infinity Cache cannot hold
    if (patch == 0) lnb_launch<384, 0>(g, stream);
    else if (C == 96) lnb_launch<96, 1>(g, stream);
    else if (C == 192) lnb_launch<192, 1>(g, stream);
    else lnb_launch<384, 1>(g, stream);
    MMG_LAUNCH_CHECK("mmg_gemm_nt_lnbwd");
    return 0;
}
