// Host-side planning of the five GEMM doors (mmg_gemm_nt_bf16 / _nt_fp8 / _nt_fp8_bwd / _tn_bf16 / _tn_fp8): argument checks, the
// tuning knobs, and for every launch ONE plan - which kernel instantiation, on what grid, with how much LDS, and the derived fields the
// kernel reads.  Pure integer arithmetic: no HIP call and no kernel file, so the rules compile in a second and are pinned by a CPU test
// (tests/test_gemm_plan_cpu.py, through the read-only door mmg_gemm_plan).  gemm_bf16.hip, gemm_tn_wide.hip and gemm_tn_fp8.hip validate,
// plan, and launch what the plan names.
#pragma once

// ---- the kernel instantiations.  Ids, the names mmg_last_kernel() reports and the launch switches of the kernel files are all
// generated from these tables, so a plan cannot name a kernel that is not built, nor a note differ from the plan. ----------------------
#define GEMM_NT_KERNELS(X) /* gemm_nt_kernel<BM, BN, BK, WAVES_M, NST, F8>   (gemm_bf16.hip) */                                     \
    X(128, 128, 64, 2, 2, 0) X(128, 128, 32, 2, 2, 0) X(128, 128, 32, 2, 3, 0) X(128, 96, 64, 2, 2, 0) X(128, 96, 32, 2, 2, 0)     \
    X(256, 256, 64, 4, 2, 0) X(256, 192, 64, 4, 2, 0) X(256, 128, 64, 4, 3, 0)                                                     \
    X(128, 128, 64, 2, 2, 1) X(256, 256, 64, 4, 2, 1) X(256, 128, 64, 4, 3, 1) X(128, 128, 64, 2, 2, 2) X(256, 256, 64, 4, 2, 2)
#define GEMM_TN_KERNELS(X) /* gemm_tn_kernel<K1, K2, BK>: (128 K1) x (128 K2) tiles, stages of BK rows   (gemm_bf16.hip) */        \
    X(1, 1, 64) X(1, 2, 32) X(2, 1, 32)
#define GEMM_TW_KERNELS(X) /* gemm_tn_wide_kernel<T1, T2> and its TwCfg<T1, T2>::FM, in the order the least-padding search prefers them */ \
    X(192, 384, 6) X(256, 256, 8) X(96, 384, 6) X(128, 256, 4)
#define GEMM_T8_KERNELS(X) /* gemm_tn8_kernel<AF>: 128 x 128 tiles; AF 1 = A in e5m2   (gemm_tn_fp8.hip) */ X(0) X(1)
#define GEMM_W8_KERNELS(X) /* gemm_tn8_wide_kernel<AF>: 256 x 256 tiles */ X(0) X(1)

enum GemmKernel {
    GK_NONE = 0,
#define X(BM, BN, BK, WM, NST, F8) GK_NT_##BM##_##BN##_##BK##_##WM##_##NST##_##F8,
    GEMM_NT_KERNELS(X)
#undef X
#define X(K1, K2, BK) GK_TN_##K1##_##K2##_##BK,
    GEMM_TN_KERNELS(X)
#undef X
#define X(T1, T2, FM) GK_TW_##T1##_##T2,
    GEMM_TW_KERNELS(X)
#undef X
#define X(AF) GK_T8_##AF,
    GEMM_T8_KERNELS(X)
#undef X
#define X(AF) GK_W8_##AF,
    GEMM_W8_KERNELS(X)
#undef X
    GK_COUNT
};
const char* gemm_kernel_name(int kernel);      // as rocprofv3's kernel trace spells it: "gemm_nt_kernel<256, 256, 64, 4, 2, 0>"
int gemm_kernel_stage_rows(int kernel);        // weight-gradient kernels: reduction rows per LDS stage (rows_per_chunk is a multiple); NT: 0

// ---- tuning knobs (A/B switches kept from the measurements in DESIGN.md / profiles/; not needed in normal use) ------------------------
struct GemmKnobs {
    // read ONCE per process, at the first GEMM call
    int gemm_bk;            // MMG_GEMM_BK          0      32: never the 64-column stages
    int gemm_v2;            // MMG_GEMM_V2          1      0: no 256 x 128 tile
    int gemm_nt_store;      // MMG_GEMM_NT_STORE   -1      0 / 1 forces the streaming stores of mmg_gemm_nt_bf16 off / on
    int gemm_3wg;           // MMG_GEMM_3WG         1      0: no three-workgroup tile at short K
    int gemm_k3;            // MMG_GEMM_K3        128      the three-workgroup tile below this K
    int gemm_kbig;          // MMG_GEMM_KBIG     4096      the 256 x 128 tile from this K
    int gemm_256;           // MMG_GEMM_256       384      the 256 x 256 tile from this K (0 = never)
    int gemm_fill;          // MMG_GEMM_FILL        1      0: 256-row tiles whatever their last round of CUs looks like
    int fp8_tile;           // MMG_FP8_TILE         0      mmg_gemm_nt_fp8: 1 = 256 x 128 at most, 2 = 128 x 128 only
    int tn_wgs;             // MMG_TN_WGS         512      workgroup budget of gemm_tn_kernel (two per CU)
    int tn_xcd;             // MMG_TN_XCD           1      0: plain (tile, chunk) grid
    int tn_wide;            // MMG_TN_WIDE          1      0: no 256-wide tiles of gemm_tn_kernel
    int tn_wide8_min_m;     // MMG_TN_WIDE8_MIN_M 65536    shortest reduction that takes gemm_tn_wide_kernel
    int tn_wide_b;          // MMG_TN_WIDE_B        1      0: gemm_tn_wide_kernel without its 256-wide tiles
    int tn8_wgs;            // MMG_TN8_WGS       1024      workgroup budget of gemm_tn8_kernel (two per CU, two rounds)
    // read on EVERY call of the door that uses them: tests and tools set them inside one process
    int gemm_192;           // MMG_GEMM_192       384      the 256 x 192 tile from this K (0 = never); tools/nt_192_ab.py
    int tn_wide8;           // MMG_TN_WIDE8         1      0: mmg_gemm_tn_bf16 stays on gemm_tn_kernel
    int tn8_wide;           // MMG_TN8_WIDE        -1      0 / 1 forces the 128 x 128 / 256 x 256 tiles of mmg_gemm_tn_fp8
    int tn8_xcd;            // MMG_TN8_XCD          1      0: gemm_tn8_kernel on a plain (tile, chunk) grid
};
enum { GEMM_LIVE_NT = 1, GEMM_LIVE_TN = 2, GEMM_LIVE_TN8 = 4 };
// the cached knobs, plus a fresh read of the per-call ones of the named doors (the others keep their defaults)
GemmKnobs gemm_knobs(int live);

// ---- one plan per launch ---------------------------------------------------------------------------------------------------------------
struct GemmPlan {
    int kernel;                         // GemmKernel
    int grid_x, grid_y, block, lds;     // lds: dynamic LDS bytes
    int tiles1, tiles2;                 // NT: tiles_m, tiles_n;  TN: tiles over N1, N2 (after the exchange when `swapped`)
    int chunks, rows_per_chunk;         // TN: split of the reduction
    int xcd;                            // gemm_tn_kernel: xcd_order;  gemm_tn8_*: xcd_map;  0 elsewhere
    int xcd_split;                      // gemm_tn8_*: S of t8_xcd_map
    int swapped;                        // gemm_tn_wide_kernel: operands exchanged, tile flushed transposed
};
enum GemmNTKind { GEMM_NT_BF16 = 0, GEMM_NT_FP8 = 1, GEMM_NT_FP8_BWD_E5M2 = 2, GEMM_NT_FP8_BWD_E4M3 = 3 };   // = op of mmg_gemm_plan
// K as the door receives it (elements of A: bytes for the fp8 kinds)
GemmPlan plan_nt(int kind, int M, int N, int K, const GemmKnobs& kn);
int plan_nt_store(int kind, int M, int N, int out_bytes, const GemmKnobs& kn);   // GemmNT::nt_store
GemmPlan plan_tn(int M, int N1, int N2, const GemmKnobs& kn);
GemmPlan plan_tn8(int a_e5m2, int M, int N1, int N2, int cus, const GemmKnobs& kn);

// ---- one validated argument path per family: non-zero = rejected, the message (mmg_last_error) starts with the door's name --------------
enum { EPI_NONE = 0, EPI_GELU = 1, EPI_DGELU = 2, EPI_RELU = 3, EPI_DRELU = 4, EPI_DGELU_ONLY = 5, EPI_GELU_DAUX = 6, EPI_MUL_AUX = 7 };
enum { GEMM_OUT_BF16 = 0, GEMM_OUT_F32 = 1, GEMM_OUT_E4M3 = 2, GEMM_OUT_E5M2 = 3 };
struct GemmNTArgs {
    const void* A; int lda; const void* B; int ldb; void* C; int ldc; int M, N, K;
    const float* bias; const float* colscale; const void* residual; int ldr;
    const void* aux_in; int ldai; void* aux_out; int ldao;
    int epi, out_kind; float alpha; const float* alpha_dev; const float* alpha_dev2;
};
struct GemmTNArgs { const void* A; int lda; const void* B; int ldb; float* C; int ldc; int M, N1, N2; };
const char* gemm_nt_door(int kind);                      // "mmg_gemm_nt_bf16" ...
int gemm_nt_elem_bytes(int kind);                        // size of an A / B element: K, lda, ldb count these
int gemm_nt_check(int kind, const GemmNTArgs& a);
const char* gemm_tn_door(int fp8);
int gemm_tn_check(int fp8, const GemmTNArgs& a);
