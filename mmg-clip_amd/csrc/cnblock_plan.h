// Host-side planning of the five fused-CNBlock doors (mmg_cnblock_mlp_fwd / _mlp_bwd / mmg_cnblock_bwdw and the two weight-packing doors
// mmg_cnblock_pack_weights / mmg_cnblock_bwdw_pack): the per-width constants, the argument checks, the five A/B knobs, and for every launch
// ONE plan - which kernel instantiation (cnblock_bwdw: two), on how many workgroups of how many threads, with how much LDS, over how many
// tiles, with or without streaming stores.  Pure integer arithmetic: no HIP call and no kernel, so the rules are pinned by a CPU test
// (tests/test_cnblock_plan_cpu.py, through the read-only door mmg_cnblock_plan).  cnblock_mlp.hip and cnblock_bwdw.hip validate, plan, and
// launch what the plan names.
#pragma once
#include "common.h"

// ---- the per-width constants: MlpCfg<C> (cnblock_mlp.hip), BwCfg<C> (cnblock_bwdw.hip) and cn_plan all read these --------------------------
// Work split of cnblock_mlp per width.  Up to C = 256 a wave owns 32 rows (two 16-row MFMA tiles share every weight fragment read); at
// C = 384 and beyond the per-row state (C/4 operand + C/4 accumulator registers per tile) only leaves room for one tile per wave, so the
// workgroup is 8 waves of 16 rows (one workgroup per CU) and the kernel is LDS-read bound (one fragment read per MFMA).
struct CnCfg {
    int NC;                 // hidden columns per streamed chunk
    int MT;                 // 16-row tiles per wave
    int WAVES;
    int BM;                 // rows per workgroup tile
    int WGS, WGS_BWD;       // forward / backward workgroups per CU (registers / LDS)
};
constexpr CnCfg cn_cfg(int C) {
    return {C <= 128 ? 64 : 32, C <= 256 ? 2 : 1, C <= 256 ? 4 : 8, (C <= 256 ? 4 : 8) * 16 * (C <= 256 ? 2 : 1),
            C <= 96 ? 3 : (C <= 192 ? 2 : 1), C <= 192 ? 2 : 1};
}
constexpr bool cn_mlp_supported(int C) { return C == 96 || C == 128 || C == 192 || C == 256 || C == 384 || C == 512; }
// mmg_cnblock_mlp_bwd: 1 = hidden row recomputed (forward saves nothing 4C-wide), 2 = needs the forward's saved pre-activation, 0 = unsupported
constexpr int cn_mlp_bwd_mode(int C) { return (C == 96 || C == 128 || C == 192) ? 1 : (C == 384 ? 2 : 0); }

// cnblock_bwdw: rows per tile, dynamic LDS bytes (BwCfg<C> lays them out and asserts that it fills exactly this) and bf16 elements of the
// packed weight buffer: [W1 LDS image][W1 gamma fragments][gamma_ls W2^T fragments]
struct CnBwCfg { int R; int LDS; long PK_TOTAL; };
constexpr CnBwCfg cn_bw_cfg(int C) {
    // W1 image and dh image at a hidden pitch of 4C + 8, two row images at a pitch of R + 8, ln_w [C], b1' [4C], row statistics [2][R][2]
    return {64, (C / 8) * (4 * C + 8) * 16 + 2 * (C / 8) * (64 + 8) * 16 + (64 / 16) * 4 * (4 * C + 8) * 8 + C * 4 + 4 * C * 4 + 2 * 64 * 2 * 4,
            (long)(C / 8) * (4 * C + 8) * 8 + 2 * (long)(4 * C / 16) * (C / 32) * 64 * 8};
}
constexpr bool cn_bwdw_supported(int C) { return C == 96; }

// ---- the kernel instantiations: F(C, SAVE) = cnblock_mlp_fwd_kernel<C, SAVE>, R(C, RW) = cnblock_mlp_fwd_kernel<C, false, RW> (resident
// weights), B(C, RECOMP, LNB) = cnblock_mlp_bwd_kernel<C, RECOMP, LNB>, W(C, MODE, NW, VAR) = cnblock_bwdw_kernel<C, MODE, NW, VAR>.  Ids, the
// names mmg_last_kernel() reports and the launch switches of the two kernel files are all generated from this table: nothing is built that
// it does not list (one row per kernel family, so that a launch switch expands its own), and a plan outside it has no name and is refused. --
#define CN_FWD_KERNELS(F, R)                                                                                                        \
    F(96, false) F(96, true) F(128, false) F(128, true) F(192, false) F(192, true)                                                  \
    F(256, false) F(256, true) F(384, false) F(384, true) F(512, false) F(512, true) R(96, 8) R(96, 12)
#define CN_BWD_KERNELS(B)                                                                                                           \
    B(96, true, false) B(96, true, true) B(128, true, false) B(128, true, true)                                                     \
    B(192, true, false) B(192, true, true) B(384, false, false) B(384, false, true)
#define CN_BWDW_KERNELS(W) W(96, 1, 8, 0) W(96, 1, 8, 1) W(96, 1, 8, 2) W(96, 1, 12, 0) W(96, 2, 8, 0) W(96, 2, 8, 1)
#define CN_KERNELS(F, R, B, W) CN_FWD_KERNELS(F, R) CN_BWD_KERNELS(B) CN_BWDW_KERNELS(W)

enum { CN_FAM_fwd = 0, CN_FAM_bwd = 1, CN_FAM_bwdw = 2 };
// an id is its instantiation, packed (never 0).  fwd: A = SAVE, B = RW;  bwd: A = RECOMP, B = LNB;  bwdw: A = MODE, B = NW, V = VAR
#define CN_KEY(FAM, C, A, B, V) (((((FAM) * 1024 + (C)) * 4 + (A)) * 16 + (B)) * 4 + (V))
enum CnKernel {
#define KF(C, SAVE) CK_fwd_##C##_##SAVE = CN_KEY(CN_FAM_fwd, C, SAVE, 0, 0),
#define KR(C, RW) CK_fwd_##C##_res##RW = CN_KEY(CN_FAM_fwd, C, 0, RW, 0),
#define KB(C, RECOMP, LNB) CK_bwd_##C##_##RECOMP##_##LNB = CN_KEY(CN_FAM_bwd, C, RECOMP, LNB, 0),
#define KW(C, MODE, NW, VAR) CK_bwdw_##C##_##MODE##_##NW##_##VAR = CN_KEY(CN_FAM_bwdw, C, MODE, NW, VAR),
    CN_KERNELS(KF, KR, KB, KW)
#undef KF
#undef KR
#undef KB
#undef KW
};
const char* cn_kernel_name(int kernel);        // as rocprofv3's kernel trace spells it: "cnblock_mlp_fwd_kernel<96, false, 12>"; "" when not in the table

// ---- the doors ------------------------------------------------------------------------------------------------------------------------------
enum CnDoorId { CN_FWD = 0, CN_BWD = 1, CN_BWDW = 2, CN_PACK = 3, CN_BWDW_PACK = 4, CN_DOORS = 5 };   // 0 .. 2 = op of mmg_cnblock_plan

// ---- tuning knobs (A/B switches; tools/mlp_fwd_res_ab.py, tools/bwdw_bench.py).  Read on EVERY call: tests and those tools set them inside
// one process.  The raw values: cn_plan applies the fallbacks of out-of-range ones. ------------------------------------------------------
struct CnKnobs {
    int fwd_res;            // MMG_MLP_FWD_RES    12     waves per workgroup of the resident forward (C = 96, nothing saved): 8 / 12; else streaming
    int nt_store;           // MMG_MLP_NT_STORE   -1     unset: by rule (cn_plan); 0 / 1: the 4C-wide stores plain / past L2 everywhere
    int bwdw_var;           // MMG_BWDW_VAR       2      schedule of cnblock_bwdw's launch 1: 1 / 2; else 0
    int bwdw_hto;           // MMG_BWDW_HTO       1      launch 2 in the ht-outer step order; 0: off
    int bwdw_w12;           // MMG_BWDW_W12       0      launch 1 with 12 waves (and schedule 0)
};
CnKnobs cn_knobs();

// ---- what the checks read (a door leaves what it does not take at zero) ------------------------------------------------------------------
struct CnArgs {
    long long M; int C;
    int operands;                                       // every pointer the door requires is given
    const void *hpre, *xln, *gact, *mean, *rstd;        // mmg_cnblock_mlp_fwd's optional outputs (hpre: also mmg_cnblock_mlp_bwd's optional input)
    int hpre_kind;
    const void *ln_dw, *ln_db;                          // mmg_cnblock_mlp_bwd's optional pair
    int backward; const void* gamma;                    // mmg_cnblock_pack_weights
};
// one validated argument path: non-zero = rejected, the message (mmg_last_error) starts with the door's name
int cn_check(int door, const CnArgs& a);

// ---- one plan per launch (cnblock_bwdw: per pair of launches) ---------------------------------------------------------------------------------
struct CnPlan {
    int kernel, kernel2;            // CnKernel; kernel2: cnblock_bwdw's launch 2, else 0
    int tile;                       // rows per walked tile: a workgroup's (BM, 64) or, in the resident forward, a wave's (32)
    int ntiles;
    int grid, block, block2, lds;   // workgroups (both launches), threads (launch 1, launch 2), dynamic LDS bytes
    int nt;                         // the 4C-wide outputs are stored past L2
};
// door: CN_FWD / CN_BWD / CN_BWDW, a shape cn_check has passed.  save: the forward saves hpre (+ statistics);  ln: the backward gets ln_dw / ln_db
CnPlan cn_plan(int door, long long M, int C, int save, int ln, int cus, const CnKnobs& kn);
const char* cn_plan_name(const CnPlan& p);     // what mmg_last_kernel() reports: the kernel's name; cnblock_bwdw: "cnblock_bwdw_kernel<..> + <..>"
