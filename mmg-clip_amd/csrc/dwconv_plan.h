// Host-side planning of the three depthwise 7x7 doors (mmg_dwconv7_nhwc / mmg_dwconv7_nhwc_mfma / mmg_dwconv7_wgrad): the tile and LDS
// constants the host arithmetic shares with the kernels, the argument checks, the five A/B knobs, and for every launch ONE plan - which
// kernel instantiation, on which grid of how many threads, with how much LDS, over which tiles, with or without streaming stores.  Pure
// integer arithmetic: no HIP call and no kernel, so the rules are pinned by a CPU test (tests/test_dwconv_plan_cpu.py, through the
// read-only door mmg_dwconv7_plan).  dwconv7.hip and dwconv7_mfma.hip validate, plan, and launch what the plan names.
#pragma once
#include "common.h"

// ---- the VALU kernels' tile (dwconv7.hip): a workgroup owns a TH x 32 pixel tile of a 32-channel slab --------------------------------------
#define DW_TW 32
#define DW_TH 8
#define DW_CB 32
#define DW_COLS (DW_TW + 6)
#define DW_ROWS (DW_TH + 6)
#define DW_ROWD (DW_COLS * (DW_CB / 2) + 16)   // dwords per LDS row; +16 keeps rows r, r+1 on disjoint bank halves
// DW_TH = 8 keeps the tile at 34 KiB so four workgroups share a CU (latency hiding for the LDS-read / FMA phases)
// two-rows-per-lane kernels: the row pitch is 616 dwords so that the four row groups of a wave, now two rows apart, still start 16 banks apart
#define DW_ROWD2 (DW_COLS * (DW_CB / 2) + 8)
#define DW_FWD_TH_DEFAULT 8

// ---- the matrix-core kernel's LDS layout (dwconv7_mfma.hip) ---------------------------------------------------------------------------------
#define DM_T 16                              // output tile edge
#define DM_H 22                              // halo tile edge
#define DM_CB 32                             // channels per slab (64 contiguous bytes per pixel)
#define DM_NPIX (DM_H * DM_H)                // 484
#define DM_CHUNKS 2048                       // 16-byte chunks a workgroup moves per halo tile (4 per thread; 1936 carry pixels)
#define DM_IN_BYTES (DM_CHUNKS * 16)         // the NHWC halo tile (the transposed reads of a row's last column group run 2 pixels over: inside)
#define DM_ROWB 96                           // bytes per plane row (48 bf16: x_in 0..21 data, 22..31 read by the MFMA against zero taps)
#define DM_PLANE (DM_H * DM_ROWB + 16)       // 2128
#define DM_PLANAR (DM_CB * DM_PLANE)         // 68 096
#define DM_OROWB 40                          // a channel's 16 x 16 outputs go back into ITS OWN (consumed) input plane: 40-byte rows
#define DM_OPIX 80                           // bytes per pixel of the NHWC output tile
#define DM_OUT_BYTES (DM_T * DM_T * DM_OPIX)
#define DM_OFF_IN 0
#define DM_OFF_PLANAR DM_IN_BYTES
#define DM_OFF_OUT (DM_OFF_PLANAR + DM_PLANAR)
#define DM_LDS (DM_OFF_OUT + DM_OUT_BYTES)
// ADD instantiations carry the fp32 accumulators to the output pass WHOLE, as two 16-bit halves through the same 16-bit transposes: the high
// halves take the path of the bf16 outputs, the low halves go D -> the (consumed) NHWC input tile region, planes DM_LO_PLANE apart (= DM_PLANE
// mod 256: the bank pattern of the high halves) -> E -> a second NHWC output tile.  F rebuilds the fp32 value, adds the residual operand and
// rounds ONCE, as the VALU kernels do (rounding conv + bias to bf16 first and the sum again was off by up to half an ulp of the LARGER of the two).
#define DM_LO_PLANE 848
#define DM_OFF_OUT_LO (DM_OFF_OUT + DM_OUT_BYTES)
#define DM_LDS_ADD (DM_OFF_OUT_LO + DM_OUT_BYTES)
static_assert(DM_LDS_ADD <= 160 * 1024, "LDS budget");
static_assert(DM_LO_PLANE >= DM_T * DM_OROWB && DM_CB * DM_LO_PLANE <= DM_IN_BYTES && DM_LO_PLANE % 16 == 0, "the low halves fit the input tile region");
static_assert(DM_PLANE % 16 == 0 && DM_T * DM_OROWB <= DM_PLANE, "alignment / the output rows fit the plane they replace");
static_assert(DM_CB == DW_CB, "one slab width for the three doors");

// ---- the kernel instantiations: V(FLIP) = dwconv7_kernel<FLIP>, R(FLIP, TH) = dwconv7_rows2_kernel<FLIP, TH>, M(FLIP, NW, ADD) =
// dwconv7_mfma_kernel<FLIP, NW, ADD>, G() = dwconv7_wgrad_kernel, G2(TH) = dwconv7_wgrad_rows2_kernel<TH>.  Ids, the names mmg_last_kernel()
// reports and the launch switches of the two kernel files are all generated from this table (one row per door, so that a launch switch
// expands its own): nothing is launched that it does not list, and a plan outside it has no name and is refused. ---------------------------
#define DW_FWD_KERNELS(V, R) V(false) V(true) R(false, 8) R(false, 16) R(true, 8) R(true, 16)
#define DW_MFMA_KERNELS(M)                                                                                                          \
    M(false, 8, false) M(false, 8, true) M(false, 16, false) M(false, 16, true)                                                     \
    M(true, 8, false) M(true, 8, true) M(true, 16, false) M(true, 16, true)
#define DW_WGRAD_KERNELS(G, G2) G() G2(8) G2(16)
#define DW_KERNELS(V, R, M, G, G2) DW_FWD_KERNELS(V, R) DW_MFMA_KERNELS(M) DW_WGRAD_KERNELS(G, G2)

enum { DW_FAM_fwd = 1, DW_FAM_rows2 = 2, DW_FAM_mfma = 3, DW_FAM_wgrad = 4, DW_FAM_wgrad2 = 5 };
// an id is its instantiation, packed (never 0).  T: tile height (rows2 kernels) or waves per workgroup (matrix cores)
#define DW_KEY(FAM, FLIP, T, ADD) (((((FAM) * 2 + (FLIP)) * 32 + (T)) * 2) + (ADD))
enum DwKernel {
#define KV(FLIP) DK_fwd_##FLIP = DW_KEY(DW_FAM_fwd, FLIP, 0, 0),
#define KR(FLIP, TH) DK_rows2_##FLIP##_##TH = DW_KEY(DW_FAM_rows2, FLIP, TH, 0),
#define KM(FLIP, NW, ADD) DK_mfma_##FLIP##_##NW##_##ADD = DW_KEY(DW_FAM_mfma, FLIP, NW, ADD),
#define KG() DK_wgrad = DW_KEY(DW_FAM_wgrad, 0, 0, 0),
#define KG2(TH) DK_wgrad2_##TH = DW_KEY(DW_FAM_wgrad2, 0, TH, 0),
    DW_KERNELS(KV, KR, KM, KG, KG2)
#undef KV
#undef KR
#undef KM
#undef KG
#undef KG2
};
// what mmg_last_kernel() reports: "dwconv7_rows2_kernel<false, 8>"; the matrix-core note does not spell ADD ("dwconv7_mfma_kernel<false, 16>":
// recorded launches and the traffic tools key on it); "" when not in the table
const char* dw_kernel_name(int kernel);

// ---- the doors (= op of mmg_dwconv7_plan) ---------------------------------------------------------------------------------------------------
enum DwDoorId { DW_NHWC = 0, DW_MFMA = 1, DW_WGRAD = 2, DW_DOORS = 3 };

// ---- tuning knobs (A/B switches; tools/dw_fwd_ab.py, tools/dw_wgrad_ab.py).  Read on EVERY call: tests and those tools set them inside one
// process.  The raw values: dw_plan applies the fallbacks of out-of-range ones. -------------------------------------------------------------
struct DwKnobs {
    int rows2;              // MMG_DWCONV_ROWS2   1      the two-rows-per-lane VALU kernels (forward and weight gradient); 0: the one-row kernels
    int fwd_th;             // MMG_DWCONV_TH      8      tile height of the rows2 forward: 16; else 8
    int wgrad_th;           // MMG_DWG_TH         0      tile height of the rows2 weight gradient: 8 / 16; else by rule (dw_plan)
    int wgrad_align;        // MMG_DWG_ALIGN      1      weight-gradient workgroups per slab rounded down to a multiple of 8; 0: off
    int mfma_waves;         // MMG_DWM_WAVES      16     waves per workgroup of the matrix-core kernel: 8; else 16
};
DwKnobs dw_knobs();

// ---- what the checks read ---------------------------------------------------------------------------------------------------------------------
struct DwArgs {
    int n, H, W, C;
    int operands;           // every pointer the door requires is given
};
// one validated argument path: non-zero = rejected, the message (mmg_last_error) starts with the door's name
int dw_check(int door, const DwArgs& a);

// ---- one plan per launch ------------------------------------------------------------------------------------------------------------------------
struct DwPlan {
    int kernel;                     // DwKernel
    int th, tw;                     // tile height and width in pixels
    int tiles_w, tiles_h;
    long long items;                // n * tiles_w * tiles_h: the (image, tile) pairs of one slab
    int slabs;                      // C / 32
    int gx, gy, gz, block, lds;     // grid, threads, dynamic LDS bytes
    int nt;                         // the output is stored past L2 (never the weight gradient: it has no activation-sized output)
    unsigned m_img, m_tw;           // matrix cores: floor(2^32 / (tiles_w * tiles_h)), floor(2^32 / tiles_w) (divisors below 2: 2)
    int by_image;                   // matrix cores, informational (the kernel computes it itself): n >= 8, an image belongs to one XCD group
};
// door: a shape dw_check has passed.  flip, add: forward doors only;  cus: matrix-core door only
DwPlan dw_plan(int door, int n, int H, int W, int C, int flip, int add, int cus, const DwKnobs& kn);
