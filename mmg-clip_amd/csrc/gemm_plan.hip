// Host-only half of the GEMM doors (see gemm_plan.h): knobs, argument checks, kernel selection, grids and LDS sizes, and the read-only
// door mmg_gemm_plan.  No HIP call, no kernel: what a launch will be is decided here and can be asked for without launching.
#include "common.h"
#include "gemm_plan.h"
#include <stdlib.h>
#include <string.h>

// ---- kernel tables ------------------------------------------------------------------------------------------------------------------------
static const char* const kKernelNames[GK_COUNT] = {
    "",
#define X(BM, BN, BK, WM, NST, F8) "gemm_nt_kernel<" #BM ", " #BN ", " #BK ", " #WM ", " #NST ", " #F8 ">",
    GEMM_NT_KERNELS(X)
#undef X
#define X(K1, K2, BK) "gemm_tn_kernel<" #K1 ", " #K2 ", " #BK ">",
    GEMM_TN_KERNELS(X)
#undef X
#define X(T1, T2, FM) "gemm_tn_wide_kernel<" #T1 ", " #T2 ">",
    GEMM_TW_KERNELS(X)
#undef X
#define X(AF) "gemm_tn8_kernel<" #AF ">",
    GEMM_T8_KERNELS(X)
#undef X
#define X(AF) "gemm_tn8_wide_kernel<" #AF ">",
    GEMM_W8_KERNELS(X)
#undef X
};
const char* gemm_kernel_name(int kernel) { return kernel > GK_NONE && kernel < GK_COUNT ? kKernelNames[kernel] : ""; }

struct NtTile { int bm, bn, bk, waves_m, nst; };
static const NtTile kNtTiles[] = {
#define X(BM, BN, BK, WM, NST, F8) {BM, BN, BK, WM, NST},
    GEMM_NT_KERNELS(X)
#undef X
};
static const int kTnTiles[][3] = {
#define X(K1, K2, BK) {K1, K2, BK},
    GEMM_TN_KERNELS(X)
#undef X
};
static const int kTwTiles[][3] = {
#define X(T1, T2, FM) {T1, T2, FM},
    GEMM_TW_KERNELS(X)
#undef X
};
enum { GK_NT_FIRST = GK_NONE + 1, GK_TN_FIRST = GK_TN_1_1_64, GK_TW_FIRST = GK_TW_192_384, GK_T8_FIRST = GK_T8_0, GK_W8_FIRST = GK_W8_0 };
enum { TN_T = 128, TW_BK = 32, TW_NS = 4, TW_IMG = TW_BK * 128, T8_T = 128, T8_BK = 128, W8_T = 256 };   // tile constants of the kernel files

int gemm_kernel_stage_rows(int kernel) {
    if (kernel >= GK_T8_FIRST && kernel < GK_COUNT) return T8_BK;
    if (kernel >= GK_TW_FIRST && kernel < GK_T8_FIRST) return TW_BK;
    if (kernel >= GK_TN_FIRST && kernel < GK_TW_FIRST) return kTnTiles[kernel - GK_TN_FIRST][2];
    return 0;
}

// ---- knobs ----------------------------------------------------------------------------------------------------------------------------------
static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
GemmKnobs gemm_knobs(int live) {
    static const GemmKnobs cached = [] {
        GemmKnobs k;
        k.gemm_bk = env_int("MMG_GEMM_BK", 0);
        k.gemm_v2 = env_int("MMG_GEMM_V2", 1);
        k.gemm_nt_store = env_int("MMG_GEMM_NT_STORE", -1);
        k.gemm_3wg = env_int("MMG_GEMM_3WG", 1);
        k.gemm_k3 = env_int("MMG_GEMM_K3", 128);
        k.gemm_kbig = env_int("MMG_GEMM_KBIG", 4096);
        k.gemm_256 = env_int("MMG_GEMM_256", 384);
        k.gemm_fill = env_int("MMG_GEMM_FILL", 1);
        k.fp8_tile = env_int("MMG_FP8_TILE", 0);
        k.tn_wgs = env_int("MMG_TN_WGS", 512);
        k.tn_xcd = env_int("MMG_TN_XCD", 1);
        k.tn_wide = env_int("MMG_TN_WIDE", 1);
        k.tn_wide8_min_m = env_int("MMG_TN_WIDE8_MIN_M", 65536);
        k.tn_wide_b = env_int("MMG_TN_WIDE_B", 1);
        k.tn8_wgs = env_int("MMG_TN8_WGS", 1024);
        k.gemm_192 = 384; k.tn_wide8 = 1; k.tn8_wide = -1; k.tn8_xcd = 1;
        return k;
    }();
    GemmKnobs k = cached;
    if (live & GEMM_LIVE_NT) k.gemm_192 = env_int("MMG_GEMM_192", 384);
    if (live & GEMM_LIVE_TN) k.tn_wide8 = env_int("MMG_TN_WIDE8", 1);
    if (live & GEMM_LIVE_TN8) {
        const char* ew = getenv("MMG_TN8_WIDE");
        k.tn8_wide = ew ? atoi(ew) != 0 : -1;
        k.tn8_xcd = env_int("MMG_TN8_XCD", 1);
    }
    return k;
}

// ---- NT --------------------------------------------------------------------------------------------------------------------------------------
static GemmPlan nt_plan_for(int kernel, int M, int N) {
    const NtTile& t = kNtTiles[kernel - GK_NT_FIRST];
    GemmPlan p = {};
    p.kernel = kernel;
    p.tiles1 = cdiv(M, t.bm);
    p.tiles2 = cdiv(N, t.bn);
    p.grid_x = p.tiles1 * p.tiles2;
    p.grid_y = 1;
    p.block = t.waves_m * 128;
    const size_t stage = (size_t)t.nst * (t.bm * t.bk * 2 + t.bn * t.bk * 2);
    const size_t cs = (size_t)64 * (t.bn + 4) * 4;
    p.lds = (int)(stage > cs ? stage : cs);
    return p;
}

static int nt_kernel_bf16(int M, int N, int K, const GemmKnobs& kn) {
    const bool k64 = (K % 64 == 0) && kn.gemm_bk != 32;
    // N tile: 96 when it divides N and 128 does not (ConvNeXt widths 96/192), else 128
    const bool n96 = (N % 128 != 0) && (N % 96 == 0);
    // K < 384 (ConvNeXt stages 1-2, stem): HBM/latency bound -> 16 KiB stages, three of them, three workgroups per CU (gemm_3wg)
    // (round 2, tools/nt_knobs.py, profiles/r02_nt_tile_rules.txt: the 4.2 M x 384 x 192 data gradient of the first downsample layer ran
    // 30 % faster on the two-stage 128 x 128 x 64 tile than on the three-workgroup one, the N = 384 long-K shapes 2-4 % faster on it than
    // on 256 x 128; BERT's shapes do not care: gemm_k3, gemm_kbig)
    // 256x256 tile (8 waves, one workgroup per CU): 128 FLOP per operand byte pulled from L2, which is what bounds the
    // 128-wide tiles (~10 TB/s of L2->LDS traffic); used from K = gemm_256 upwards when N is a multiple of 256 (0 = never)
    // one workgroup per CU for the 256-row tiles: a grid that fills the last round of 256 CUs badly (BERT's ~10 k packed
    // tokens x N = 768: 123 tiles = 48 % of one round) goes to the next smaller tile when that one fills better (gemm_fill)
    auto fill = [](long wgs) { return (double)wgs / (double)(cdiv(wgs, 256) * 256L); };
    const double f256 = fill((long)cdiv(M, 256) * cdiv(N, 256)), f128 = fill((long)cdiv(M, 256) * cdiv(N, 128));
    const bool fills = !kn.gemm_fill || f256 >= 0.8 * f128;
    // (round 3, tools/nt_deep_ab.sh: the same tile on 32-column stages, three or four of them - more K tiles in flight at short K - was 2-3 %
    // SLOWER on the K = 384 / 768 fat-epilogue shapes, 2883 / 2915 against 2827 us: the main loop is not waiting for its operands.  Removed.)
    // round 4: N = 192 / 384 (ConvNeXt stage-3 d LN-out = dh W1: 1 M x 384 x 1536, 13.6 ms of a C2 step on 128 x 128 tiles at 0.33 of the MFMA peak)
    // take a 256 x 192 tile - the 256 x 256 kernel's 8 waves with 64 x 96 wave tiles (0.42 fragment reads per MFMA against 0.5): gemm_192
    const double f192 = fill((long)cdiv(M, 256) * cdiv(N, 192));
    if (kn.gemm_256 && k64 && N % 256 == 0 && M >= 4096 && K >= kn.gemm_256 && fills) return GK_NT_256_256_64_4_2_0;
    if (kn.gemm_192 && k64 && N % 192 == 0 && M >= 4096 && K >= kn.gemm_192 && (!kn.gemm_fill || f192 >= 0.8 * f128)) return GK_NT_256_192_64_4_2_0;
    if (kn.gemm_3wg && !n96 && K % 32 == 0 && K < kn.gemm_k3) return GK_NT_128_128_32_2_3_0;
    if (kn.gemm_v2 && k64 && !n96 && M >= 4096 && K >= kn.gemm_kbig) return GK_NT_256_128_64_4_3_0;
    if (n96) return k64 ? GK_NT_128_96_64_2_2_0 : GK_NT_128_96_32_2_2_0;
    return k64 ? GK_NT_128_128_64_2_2_0 : GK_NT_128_128_32_2_2_0;
}

GemmPlan plan_nt(int kind, int M, int N, int K, const GemmKnobs& kn) {
    const bool big = N % 256 == 0 && M >= 4096;
    int kernel;
    switch (kind) {
        case GEMM_NT_BF16: kernel = nt_kernel_bf16(M, N, K, kn); break;
        case GEMM_NT_FP8:                // fp8_tile: tuning, 1 = 256x128 at most, 2 = 128x128 only
            kernel = (kn.fp8_tile == 0 && big) ? GK_NT_256_256_64_4_2_1 : (kn.fp8_tile != 2 && M >= 4096) ? GK_NT_256_128_64_4_3_1 : GK_NT_128_128_64_2_2_1;
            break;
        case GEMM_NT_FP8_BWD_E5M2: kernel = big ? GK_NT_256_256_64_4_2_2 : GK_NT_128_128_64_2_2_2; break;
        default: kernel = big ? GK_NT_256_256_64_4_2_1 : GK_NT_128_128_64_2_2_1; break;
    }
    return nt_plan_for(kernel, M, N);
}

// outputs larger than the 256 MiB Infinity Cache cannot be re-read from cache anyway: stream them past L2
// (measured: -14...-20 % on the write-heavy GELU / residual epilogues); MMG_GEMM_NT_STORE=0/1 forces it off/on (mmg_gemm_nt_bf16 only)
int plan_nt_store(int kind, int M, int N, int out_bytes, const GemmKnobs& kn) {
    if (kind == GEMM_NT_BF16 && kn.gemm_nt_store >= 0) return kn.gemm_nt_store;
    return (size_t)M * N * out_bytes >= ((size_t)256 << 20);
}

// ---- TN, bf16 -------------------------------------------------------------------------------------------------------------------------------
// gemm_tn_wide_kernel when the shape suits it (kernel stays GK_NONE otherwise)
static GemmPlan plan_tn_wide(int M, int N1, int N2, const GemmKnobs& kn) {
    GemmPlan p = {};
    // every workgroup flushes a whole tile with fp32 atomics (75 MB per launch at 256 workgroups of 192 x 384 = ~60 us): only
    // reductions long enough to amortise that take this kernel
    if (M < kn.tn_wide8_min_m || N1 < 96 || N2 < 96) return p;
    const bool wide2 = N2 >= N1;                     // orientation: the wider side gets the wide tile edge (the 4 wave columns)
    const int narrow = wide2 ? N1 : N2, wideN = wide2 ? N2 : N1;
    // tile = (narrow edge, wide edge) with the least padding: 96 / 192 x 384 (ConvNeXt-T widths), 128 / 256 x 256 (ConvNeXt-B widths)
    // (largest tile first: on equal padding the bigger accumulator tile wins - 384 x 1536 runs on 192 x 384 tiles, not 96 x 384)
    const int (*cfgs)[3] = kTwTiles;
    int best = -1;
    double best_waste = 1e9;
    for (int i = 0; i < 4; ++i) {
        const double w = (double)(cdiv(narrow, cfgs[i][0]) * cfgs[i][0]) * (cdiv(wideN, cfgs[i][1]) * cfgs[i][1]) / ((double)narrow * wideN);
        if (w < best_waste - 1e-9) { best_waste = w; best = i; }
    }
    if (!kn.tn_wide_b && (best == 1 || best == 3)) { // the 256-wide tiles off: the 384-wide ones or nothing
        best = narrow <= 96 ? 2 : 0;
        best_waste = (double)(cdiv(narrow, cfgs[best][0]) * cfgs[best][0]) * (cdiv(wideN, 384) * 384) / ((double)narrow * wideN);
    }
    if (best_waste > 1.2) return p;                  // badly fitting widths stay on the 128-wide tiles of gemm_bf16.hip
    // N1 > N2 (dW1 = dh^T x of a CNBlock: [4C, C]) runs as its transpose: operands exchanged, tile flushed transposed, bias sums taken
    // from the B fragments.  (Mirrored instantiations <384, 192> / <384, 96> were equal on the stage-1/2 shapes and 2-3 % slower on
    // 1536 x 384 in a same-run A/B, profiles/r02_tn_wide_swap_ab.txt, and are gone.)
    p.swapped = !wide2;
    const int T1 = cfgs[best][0], T2 = cfgs[best][1];
    p.kernel = GK_TW_FIRST + best;
    p.tiles1 = cdiv(narrow, T1);
    p.tiles2 = cdiv(wideN, T2);
    const int ntile = p.tiles1 * p.tiles2;
    // one workgroup per CU (149 KiB of LDS): 32 per XCD = the tiles of `cpx` row chunks
    int cpx = 32 / ntile;
    if (cpx < 1) cpx = 1;
    p.chunks = 8 * cpx;
    p.rows_per_chunk = cdiv(cdiv(M, p.chunks), TW_BK) * TW_BK;
    const int NIA = (T1 + 63) / 64, NIB = (T2 + 63) / 64, FM = cfgs[best][2];
    const size_t ring = (size_t)TW_NS * (NIA + NIB) * TW_IMG;
    const size_t cs = (size_t)FM * 16 * (T2 + 4) * 4;
    p.lds = (int)(ring > cs ? ring : cs);
    p.grid_x = 8 * cpx * ntile;
    p.grid_y = 1;
    p.block = 512;
    return p;
}

GemmPlan plan_tn(int M, int N1, int N2, const GemmKnobs& kn) {
    // long reductions onto few output columns (ConvNeXt weight gradients): the 8-wave wide-tile kernel (gemm_tn_wide.hip) streams
    // both operands once per 192x384-class tile; MMG_TN_WIDE8=0 keeps gemm_tn_kernel
    if (kn.tn_wide8) {
        const GemmPlan w = plan_tn_wide(M, N1, N2, kn);
        if (w.kernel != GK_NONE) return w;
    }
    // 256-wide tiles on the wider side when it is a multiple of 256 (measured: -6...-19 % on the ConvNeXt shapes, slower on
    // the short BERT reductions where the tile count is what fills the GPU); MMG_TN_WIDE=0 disables
    const bool long_m = M >= 32768;
    GemmPlan p = {};
    if (kn.tn_wide && long_m && N2 >= N1 && N2 % 256 == 0) p.kernel = GK_TN_1_2_32;
    else if (kn.tn_wide && long_m && N1 > N2 && N1 % 256 == 0) p.kernel = GK_TN_2_1_32;
    else p.kernel = GK_TN_1_1_64;
    const int K1 = kTnTiles[p.kernel - GK_TN_FIRST][0], K2 = kTnTiles[p.kernel - GK_TN_FIRST][1], BK = kTnTiles[p.kernel - GK_TN_FIRST][2];
    const int target_wgs = kn.tn_wgs;
    p.tiles1 = cdiv(N1, K1 * TN_T);
    p.tiles2 = cdiv(N2, K2 * TN_T);
    const int tiles = p.tiles1 * p.tiles2;
    int chunks = target_wgs / tiles;
    if (chunks < 1) chunks = 1;
    const int max_chunks = cdiv(M, 64);
    if (chunks > max_chunks) chunks = max_chunks;
    p.rows_per_chunk = cdiv(cdiv(M, chunks), 64) * 64;
    chunks = cdiv(M, p.rows_per_chunk);
    p.chunks = chunks;
    p.xcd = kn.tn_xcd ? (N2 >= N1 ? 1 : 2) : 0;
    if (p.xcd) {             // whole groups per XCD: fall back when that would overfill an XCD's share of the workgroup budget
        const int G = p.xcd == 1 ? p.tiles1 : p.tiles2, ngroups = (tiles / G) * chunks;
        if (((ngroups + 7) / 8) * G * 8 > target_wgs && tiles * chunks <= target_wgs) p.xcd = 0;
    }
    const size_t stage = 2 * (size_t)(K1 + K2) * (BK * TN_T * 2);
    const size_t cs = (size_t)64 * (K2 * TN_T + 4) * 4;
    p.lds = (int)(stage > cs ? stage : cs);
    p.block = 256;
    if (p.xcd) {
        const int G = p.xcd == 1 ? p.tiles1 : p.tiles2, ngroups = (tiles / G) * chunks;
        p.grid_x = 8 * ((ngroups + 7) / 8) * G;
        p.grid_y = 1;
    } else {
        p.grid_x = tiles;
        p.grid_y = chunks;
    }
    return p;
}

// ---- TN, fp8 --------------------------------------------------------------------------------------------------------------------------------
GemmPlan plan_tn8(int a_e5m2, int M, int N1, int N2, int cus, const GemmKnobs& kn) {
    GemmPlan p = {};
    // 256 x 256 tiles (one 8-wave workgroup per CU) where both widths fill them and the reduction is long; MMG_TN8_WIDE=0 / 1 forces
    const bool wide = kn.tn8_wide >= 0 ? kn.tn8_wide != 0 : (N1 >= 256 && N2 >= 256 && M >= 8192);
    p.kernel = (wide ? GK_W8_FIRST : GK_T8_FIRST) + (a_e5m2 ? 1 : 0);
    p.xcd = wide || kn.tn8_xcd != 0;
    const int T = wide ? W8_T : T8_T;
    p.tiles1 = cdiv(N1, T);
    p.tiles2 = cdiv(N2, T);
    const int tiles = p.tiles1 * p.tiles2;
    int chunks = (wide ? cus : kn.tn8_wgs) / tiles;
    if (chunks < 1) chunks = 1;
    const int max_chunks = cdiv(M, T8_BK);
    if (chunks > max_chunks) chunks = max_chunks;
    p.rows_per_chunk = cdiv(cdiv(M, chunks), T8_BK) * T8_BK;
    p.chunks = cdiv(M, p.rows_per_chunk);
    int S = 1;                                                 // (see t8_xcd_map)
    while (S < 8 && ((p.chunks * S) % 8 != 0) && tiles % (2 * S) == 0) S *= 2;
    p.xcd_split = S;
    const int units8 = cdiv(p.chunks * S, 8) * 8;              // units are dealt in groups of 8 (workgroups past the last chunk return at once)
    if (p.xcd) { p.grid_x = (tiles / S) * units8; p.grid_y = 1; }
    else { p.grid_x = tiles; p.grid_y = p.chunks; }
    if (wide) {
        p.block = 512;
        p.lds = 2 * (2 * T8_BK * W8_T);                        // (the fp32 flush slab, 64 x 260 x 4, fits inside)
    } else {
        const size_t stage = 2 * (size_t)(2 * T8_BK * T8_T), cs = (size_t)64 * (T8_T + 4) * 4;
        p.block = 256;
        p.lds = (int)(stage > cs ? stage : cs);
    }
    return p;
}

// ---- argument checks --------------------------------------------------------------------------------------------------------------------------
struct NtDoor {
    const char* name;
    int elem;               // bytes of an A / B element
    unsigned epis, outs;    // bit e: epilogue / out_kind e is available
    const char* outs_text;
};
static const NtDoor kNtDoors[4] = {
    {"mmg_gemm_nt_bf16", 2, 0xffu, 1u << GEMM_OUT_BF16 | 1u << GEMM_OUT_F32, ""},
    {"mmg_gemm_nt_fp8", 1, 1u << EPI_NONE | 1u << EPI_GELU | 1u << EPI_RELU | 1u << EPI_GELU_DAUX,
     1u << GEMM_OUT_BF16 | 1u << GEMM_OUT_F32 | 1u << GEMM_OUT_E4M3, "0 bf16, 1 fp32, 2 e4m3"},
    {"mmg_gemm_nt_fp8_bwd", 1, 1u << EPI_NONE | 1u << EPI_DGELU_ONLY | 1u << EPI_MUL_AUX,
     1u << GEMM_OUT_BF16 | 1u << GEMM_OUT_F32 | 1u << GEMM_OUT_E5M2, "0 bf16, 1 fp32, 3 e5m2"},
};
static const NtDoor& nt_door(int kind) { return kNtDoors[kind > GEMM_NT_FP8_BWD_E5M2 ? GEMM_NT_FP8_BWD_E5M2 : kind]; }
const char* gemm_nt_door(int kind) { return nt_door(kind).name; }
int gemm_nt_elem_bytes(int kind) { return nt_door(kind).elem; }

int gemm_nt_check(int kind, const GemmNTArgs& a) {
    const NtDoor& d = nt_door(kind);
    const char* n = d.name;
    const bool f8 = d.elem == 1, bwd = kind >= GEMM_NT_FP8_BWD_E5M2;
    const int M = a.M, N = a.N, K = a.K, epi = a.epi;
    MMG_CHECK_ARG(a.A && a.B && a.C, "%s: null operand", n);
    if (bwd) {
        MMG_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % 128 == 0 && N % 8 == 0, "%s: M=%d N=%d K=%d (K a multiple of 128, N of 8)", n, M, N, K);
    } else {
        MMG_CHECK_ARG(M > 0 && N > 0 && K > 0, "%s: M=%d N=%d K=%d must be positive", n, M, N, K);
        if (f8) MMG_CHECK_ARG(K % 128 == 0, "%s: K=%d must be a multiple of 128 (one MFMA k-step)", n, K);
        else MMG_CHECK_ARG(K % 32 == 0, "%s: K=%d must be a multiple of 32", n, K);
        MMG_CHECK_ARG(N % 8 == 0, "%s: N=%d must be a multiple of 8", n, N);
    }
    if (f8) MMG_CHECK_ARG(a.out_kind >= 0 && a.out_kind < 32 && (d.outs >> a.out_kind & 1), "%s: out_kind=%d (%s)", n, a.out_kind, d.outs_text);
    const int ldm = f8 ? 16 : 8;                    // 16 bytes of A / B per row step
    const bool ld_ok = a.lda >= K && a.ldb >= K && a.ldc >= N && a.lda % ldm == 0 && a.ldb % ldm == 0 && a.ldc % 8 == 0;
    if (f8) MMG_CHECK_ARG(ld_ok, "%s: leading dimensions must cover the row; lda/ldb multiples of 16 bytes, ldc of 8 (lda=%d ldb=%d ldc=%d)", n, a.lda, a.ldb, a.ldc);
    else MMG_CHECK_ARG(ld_ok, "%s: leading dimensions must cover the row and be multiples of 8 (lda=%d ldb=%d ldc=%d)", n, a.lda, a.ldb, a.ldc);
    const bool epi_ok = epi >= 0 && epi < 32 && (d.epis >> epi & 1);
    if (f8) MMG_CHECK_ARG(epi_ok, "%s: epilogue %d not available", n, epi);
    else MMG_CHECK_ARG(epi_ok, "%s: unknown epilogue %d", n, epi);
    const bool needs_aux = epi == EPI_DGELU || epi == EPI_DGELU_ONLY || epi == EPI_DRELU || epi == EPI_MUL_AUX;
    MMG_CHECK_ARG(!needs_aux || (a.aux_in && a.ldai >= N && a.ldai % 8 == 0),
                  bwd ? "%s: the activation-gradient epilogues need aux_in" : "%s: activation-gradient epilogue needs aux_in", n);
    MMG_CHECK_ARG(!a.residual || (a.ldr >= N && a.ldr % 8 == 0), "%s: bad ldr=%d", n, a.ldr);
    MMG_CHECK_ARG(!a.aux_out || (a.ldao >= N && a.ldao % 8 == 0), "%s: bad ldao=%d", n, a.ldao);
    return 0;
}

const char* gemm_tn_door(int fp8) { return fp8 ? "mmg_gemm_tn_fp8" : "mmg_gemm_tn_bf16"; }

int gemm_tn_check(int fp8, const GemmTNArgs& a) {
    const char* n = gemm_tn_door(fp8);
    const int m = fp8 ? 16 : 8;                     // 16 bytes of A / B
    MMG_CHECK_ARG(a.A && a.B && a.C, "%s: null operand", n);
    MMG_CHECK_ARG(a.M > 0 && a.N1 >= m && a.N2 >= m, "%s: M=%d N1=%d N2=%d", n, a.M, a.N1, a.N2);
    MMG_CHECK_ARG(a.N1 % m == 0 && a.N2 % m == 0 && a.lda % m == 0 && a.ldb % m == 0 && a.lda >= a.N1 && a.ldb >= a.N2 && a.ldc >= a.N2,
                  fp8 ? "%s: N1=%d N2=%d lda=%d ldb=%d ldc=%d must be multiples of 16 (bytes) and consistent"
                      : "%s: N1=%d N2=%d lda=%d ldb=%d ldc=%d must be multiples of 8 and consistent", n, a.N1, a.N2, a.lda, a.ldb, a.ldc);
    return 0;
}

// ---- the read-only door ---------------------------------------------------------------------------------------------------------------------
MMG_API const char* mmg_gemm_plan(int op, int M, int N, int K, int cus) {
    static thread_local char text[192];
    static char dummy[16];                          // stands for the operands: the checks compare pointers with NULL and never dereference
    text[0] = 0;
    if (op < 0 || op > 6 || cus < 0) {
        mmg_set_error("mmg_gemm_plan: op=%d cus=%d (op 0..6, cus >= 0)", op, cus);
        return text;
    }
    GemmPlan p;
    if (op <= GEMM_NT_FP8_BWD_E4M3) {
        GemmNTArgs a = {};
        a.A = a.B = a.C = dummy; a.lda = a.ldb = K; a.ldc = N; a.M = M; a.N = N; a.K = K;
        if (gemm_nt_check(op, a)) return text;
        p = plan_nt(op, M, N, K, gemm_knobs(op == GEMM_NT_BF16 ? GEMM_LIVE_NT : 0));
        snprintf(text, sizeof(text), "%s grid=(%d,%d) block=%d lds=%d", gemm_kernel_name(p.kernel), p.grid_x, p.grid_y, p.block, p.lds);
        return text;
    }
    const int fp8 = op >= 5;
    const GemmTNArgs a = {dummy, N, dummy, K, (float*)dummy, K, M, N, K};
    if (gemm_tn_check(fp8, a)) return text;
    if (fp8) p = plan_tn8(op == 5, M, N, K, cus ? cus : mmg_cu_count_cached(), gemm_knobs(GEMM_LIVE_TN8));
    else p = plan_tn(M, N, K, gemm_knobs(GEMM_LIVE_TN));
    int n = snprintf(text, sizeof(text), "%s grid=(%d,%d) block=%d lds=%d chunks=%d rows=%d xcd=%d swapped=%d", gemm_kernel_name(p.kernel),
                     p.grid_x, p.grid_y, p.block, p.lds, p.chunks, p.rows_per_chunk, p.xcd, p.swapped);
    if (fp8) snprintf(text + n, sizeof(text) - n, " split=%d", p.xcd_split);
    return text;
}
