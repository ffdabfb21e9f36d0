// Host-only half of the depthwise 7x7 doors (see dwconv_plan.h): knobs, argument checks, kernel selection, grid, block and LDS size, and the
// read-only door mmg_dwconv7_plan.  No device call, no kernel: what a launch will be is decided here and can be asked for without launching.
#include "dwconv_plan.h"
#include <stdlib.h>

// ---- kernel table ---------------------------------------------------------------------------------------------------------------------------
const char* dw_kernel_name(int kernel) {
    switch (kernel) {
#define KV(FLIP) case DK_fwd_##FLIP: return "dwconv7_kernel<" #FLIP ">";
#define KR(FLIP, TH) case DK_rows2_##FLIP##_##TH: return "dwconv7_rows2_kernel<" #FLIP ", " #TH ">";
#define KM(FLIP, NW, ADD) case DK_mfma_##FLIP##_##NW##_##ADD: return "dwconv7_mfma_kernel<" #FLIP ", " #NW ">";
#define KG() case DK_wgrad: return "dwconv7_wgrad_kernel";
#define KG2(TH) case DK_wgrad2_##TH: return "dwconv7_wgrad_rows2_kernel<" #TH ">";
        DW_KERNELS(KV, KR, KM, KG, KG2)
#undef KV
#undef KR
#undef KM
#undef KG
#undef KG2
    }
    return "";
}

// ---- knobs ------------------------------------------------------------------------------------------------------------------------------------
static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
DwKnobs dw_knobs() {
    return {env_int("MMG_DWCONV_ROWS2", 1), env_int("MMG_DWCONV_TH", DW_FWD_TH_DEFAULT), env_int("MMG_DWG_TH", 0), env_int("MMG_DWG_ALIGN", 1),
            env_int("MMG_DWM_WAVES", 16)};
}

// ---- argument checks --------------------------------------------------------------------------------------------------------------------------
static const char* const dw_door_name[DW_DOORS] = {"mmg_dwconv7_nhwc", "mmg_dwconv7_nhwc_mfma", "mmg_dwconv7_wgrad"};

// the VALU kernels: the grid carries n and C / 32 in its y / z dimensions; 32-bit byte offsets inside one image, 24-bit pixel indices (dw_byte_off)
static int dw_check_valu(const char* who, int n, int H, int W, int C) {
    MMG_CHECK_ARG(n > 0 && H > 0 && W > 0 && C > 0 && C % DW_CB == 0 && n <= 65535 && C / DW_CB <= 65535,
                  "%s: n=%d H=%d W=%d C=%d (C must be a multiple of 32)", who, n, H, W, C);
    MMG_CHECK_ARG(((long long)H + 16) * ((long long)W + 64) <= (1LL << 24) && (long long)H * W * C * 2 < (1LL << 32),
                  "%s: one image of %d x %d x %d exceeds the kernels' 32-bit addressing (H * W <= 2^24, H * W * C * 2 < 2^32)", who, H, W, C);
    return 0;
}

int dw_check(int door, const DwArgs& a) {
    const int n = a.n, H = a.H, W = a.W, C = a.C;
    switch (door) {
        case DW_NHWC:
            MMG_CHECK_ARG(a.operands, "mmg_dwconv7_nhwc: null pointer");
            return dw_check_valu(dw_door_name[door], n, H, W, C);
        case DW_MFMA: {
            MMG_CHECK_ARG(a.operands, "mmg_dwconv7_nhwc_mfma: null pointer");
            MMG_CHECK_ARG(n > 0 && H > 0 && W > 0 && C > 0 && C % DM_CB == 0, "mmg_dwconv7_nhwc_mfma: n=%d H=%d W=%d C=%d (C must be a multiple of 32)", n, H, W, C);
            // The kernel forms every address as a 64-bit tile origin (scalar) + a per-thread offset held in a 32-bit int, in ELEMENTS: h_off =
            // (hr W + hc) C + part8 with hr, hc <= 21 (used when a tile's whole halo lies inside the image, so hr < H) and o_off = (r W + c) C +
            // part8 with r, c <= 15 (used for pixels inside the image, so r < H), part8 <= 24.  Both stay below min(H, 22) W C, which must
            // therefore be below 2^31: a bound on the band of rows one halo tile spans, not on the image (n and H are free: the origins are
            // 64-bit, and nothing here multiplies on the 24-bit path).  The door did not check it before.
            const int band = H < DM_H ? H : DM_H;
            MMG_CHECK_ARG((long long)W * C <= ((1LL << 31) - 1) / band,
                          "mmg_dwconv7_nhwc_mfma: %d rows of %d x %d exceed the kernel's 32-bit offsets inside a tile (min(H, 22) * W * C < 2^31)", band, W, C);
            const long long per_img = (long long)cdiv(W, DM_T) * cdiv(H, DM_T);
            MMG_CHECK_ARG(per_img < (1LL << 30) && n * per_img < (1LL << 30), "mmg_dwconv7_nhwc_mfma: too many tiles");
            return 0;
        }
        case DW_WGRAD:
            if (dw_check_valu(dw_door_name[door], n, H, W, C)) return 1;
            MMG_CHECK_ARG(a.operands, "mmg_dwconv7_wgrad: null pointer");
            return 0;
    }
    mmg_set_error("dw_check: door=%d", door);
    return 1;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
// dynamic LDS of the staged halo tile: [TH + 6][DW_ROWD2] dwords in the rows2 kernels, [DW_ROWS][DW_ROWD] in the one-row kernels
static int dw_tile_lds(int rows2, int th) { return (rows2 ? (th + 6) * DW_ROWD2 : DW_ROWS * DW_ROWD) * 4; }

DwPlan dw_plan(int door, int n, int H, int W, int C, int flip, int add, int cus, const DwKnobs& kn) {
    DwPlan p = {};
    p.slabs = C / DW_CB;
    p.gy = p.gz = 1;
    p.block = 256;
    // outputs beyond the 256 MiB Infinity Cache are stored past L2
    const int nt = (unsigned long long)n * H * W * C * 2 >= (256ULL << 20);
    const int rows2 = kn.rows2 != 0;
    if (door == DW_MFMA) {
        p.th = p.tw = DM_T;
        p.tiles_w = cdiv(W, DM_T);
        p.tiles_h = cdiv(H, DM_T);
        const int per_img = p.tiles_w * p.tiles_h;
        p.items = (long long)n * per_img;
        p.m_img = (unsigned)((1ULL << 32) / (unsigned long long)(per_img > 1 ? per_img : 2));
        p.m_tw = (unsigned)((1ULL << 32) / (unsigned long long)(p.tiles_w > 1 ? p.tiles_w : 2));
        p.by_image = n >= 8;
        p.nt = nt;
        // one workgroup per CU, a multiple of 8 (XCD groups); never fewer workgroups per XCD group than slabs
        int per_xcd = cus / 8;
        if (per_xcd < p.slabs) per_xcd = p.slabs;
        // small maps: no more streams than items
        const long long want = (p.items + 7) / 8 * p.slabs;
        if (per_xcd > want) per_xcd = (int)(want < p.slabs ? p.slabs : want);
        p.gx = 8 * per_xcd;
        const int nw = kn.mfma_waves == 8 ? 8 : 16;
        p.block = nw * 64;
        p.lds = add ? DM_LDS_ADD : DM_LDS;
        p.kernel = DW_KEY(DW_FAM_mfma, flip ? 1 : 0, nw, add ? 1 : 0);
        return p;
    }
    p.tw = DW_TW;
    p.tiles_w = cdiv(W, DW_TW);
    if (door == DW_NHWC) {
        // 16-row tiles from MMG_DWCONV_TH=16 (A/B knob; default 8), in the rows2 kernel only
        p.th = rows2 && kn.fwd_th == 16 ? 16 : DW_TH;
        p.tiles_h = cdiv(H, p.th);
        p.items = (long long)n * p.tiles_w * p.tiles_h;
        p.gx = p.tiles_w * p.tiles_h; p.gy = p.slabs; p.gz = n;
        p.lds = dw_tile_lds(rows2, p.th) + 49 * DW_CB * 4;                 // + the slab's taps [49][32]
        p.nt = nt;
        p.kernel = rows2 ? DW_KEY(DW_FAM_rows2, flip ? 1 : 0, p.th, 0) : DW_KEY(DW_FAM_fwd, flip ? 1 : 0, 0, 0);
        return p;
    }
    // weight gradient.  Tile height of the two-rows-per-lane kernel: 16 where the map is tall enough to fill the persistent grid (halo
    // 1.63x), else 8
    p.th = !rows2 ? DW_TH : (kn.wgrad_th == 8 || kn.wgrad_th == 16) ? kn.wgrad_th
                          : ((long long)n * cdiv(H, 16) * cdiv(W, DW_TW) * p.slabs >= 2048 ? 16 : 8);
    p.tiles_h = cdiv(H, p.th);
    p.items = (long long)n * p.tiles_w * p.tiles_h;
    // ~1024 workgroups in total (4 per CU), each walking its share of the (image, tile) items of one channel slab
    int per_slab = 1024 / p.slabs;
    // a multiple of 8: workgroup x of every slab then lands on XCD x % 8 (ids are x + per_slab * slab), so the slabs of one pixel - 64-byte
    // pieces of the same 128-byte lines, walked in the same order - share one L2 (measured before: 2.6x the algorithmic bytes left the L2s)
    if (kn.wgrad_align && per_slab >= 8) per_slab &= ~7;
    if (per_slab < 1) per_slab = 1;
    if (per_slab > p.items) per_slab = (int)p.items;
    p.gx = per_slab; p.gy = p.slabs;
    p.lds = dw_tile_lds(rows2, p.th) + 4 * 50 * DW_CB * 4;                 // + the reduction [4 waves][50][32]
    p.kernel = rows2 ? DW_KEY(DW_FAM_wgrad2, 0, p.th, 0) : DW_KEY(DW_FAM_wgrad, 0, 0, 0);
    return p;
}

// ---- the read-only door ---------------------------------------------------------------------------------------------------------------------
MMG_API const char* mmg_dwconv7_plan(int op, int n, int H, int W, int C, int flip, int add, int cus) {
    static thread_local char text[224];
    text[0] = 0;
    if (op < DW_NHWC || op > DW_WGRAD || cus < 0 || ((flip || add) && op == DW_WGRAD)) {
        mmg_set_error("mmg_dwconv7_plan: op=%d flip=%d add=%d cus=%d (op 0..2; flip, add: ops 0, 1; cus >= 0)", op, flip, add, cus);
        return text;
    }
    if (dw_check(op, DwArgs{n, H, W, C, 1})) return text;
    const DwPlan p = dw_plan(op, n, H, W, C, flip, add, op == DW_MFMA && !cus ? mmg_cu_count_cached() : cus, dw_knobs());
    const int len = snprintf(text, sizeof(text), "%s grid=(%d,%d,%d) block=%d lds=%d nt=%d tile=%dx%d items=%lld", dw_kernel_name(p.kernel),
                             p.gx, p.gy, p.gz, p.block, p.lds, p.nt, p.th, p.tw, p.items);
    if (op == DW_MFMA) snprintf(text + len, sizeof(text) - len, " add=%d by_image=%d", add ? 1 : 0, p.by_image);
    return text;
}
