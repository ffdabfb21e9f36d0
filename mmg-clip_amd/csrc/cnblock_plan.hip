// Host-only half of the fused-CNBlock doors (see cnblock_plan.h): knobs, argument checks, kernel selection, grid, block and LDS size, and the
// read-only door mmg_cnblock_plan.  No device call, no kernel: what a launch will be is decided here and can be asked for without launching.
#include "cnblock_plan.h"
#include <stdlib.h>

// ---- kernel table ---------------------------------------------------------------------------------------------------------------------------
const char* cn_kernel_name(int kernel) {
    switch (kernel) {
#define KF(C, SAVE) case CK_fwd_##C##_##SAVE: return "cnblock_mlp_fwd_kernel<" #C ", " #SAVE ">";
#define KR(C, RW) case CK_fwd_##C##_res##RW: return "cnblock_mlp_fwd_kernel<" #C ", false, " #RW ">";
#define KB(C, RECOMP, LNB) case CK_bwd_##C##_##RECOMP##_##LNB: return "cnblock_mlp_bwd_kernel<" #C ", " #RECOMP ", " #LNB ">";
#define KW(C, MODE, NW, VAR) case CK_bwdw_##C##_##MODE##_##NW##_##VAR: return "cnblock_bwdw_kernel<" #C ", " #MODE ", " #NW ", " #VAR ">";
        CN_KERNELS(KF, KR, KB, KW)
#undef KF
#undef KR
#undef KB
#undef KW
    }
    return "";
}

const char* cn_plan_name(const CnPlan& p) {
    static thread_local char text[96];
    if (!p.kernel2) return cn_kernel_name(p.kernel);
    const char* second = cn_kernel_name(p.kernel2);        // both launches by name; the second without the repeated "cnblock_bwdw_kernel"
    snprintf(text, sizeof(text), "%s + %s", cn_kernel_name(p.kernel), second[0] ? second + sizeof("cnblock_bwdw_kernel") - 1 : "");
    return text;
}

// ---- knobs ------------------------------------------------------------------------------------------------------------------------------------
static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
CnKnobs cn_knobs() {
    const char* nt = getenv("MMG_MLP_NT_STORE");
    return {env_int("MMG_MLP_FWD_RES", 12), nt ? (atoi(nt) != 0) : -1, env_int("MMG_BWDW_VAR", 2), env_int("MMG_BWDW_HTO", 1),
            env_int("MMG_BWDW_W12", 0)};
}

// ---- argument checks --------------------------------------------------------------------------------------------------------------------------
int cn_check(int door, const CnArgs& a) {
    const long long M = a.M;
    const int C = a.C;
    switch (door) {
        case CN_FWD:
            MMG_CHECK_ARG(a.operands, "mmg_cnblock_mlp_fwd: null pointer");
            MMG_CHECK_ARG(cn_mlp_supported(C), "mmg_cnblock_mlp_fwd: C=%d not in {96,128,192,256,384,512}", C);
            MMG_CHECK_ARG(M > 0 && M < (1LL << 36), "mmg_cnblock_mlp_fwd: bad M=%lld", M);
            MMG_CHECK_ARG((a.mean == nullptr) == (a.hpre == nullptr) && (a.rstd == nullptr) == (a.hpre == nullptr),
                          "mmg_cnblock_mlp_fwd: hpre, mean and rstd are saved together or not at all");
            MMG_CHECK_ARG(!a.xln || a.hpre, "mmg_cnblock_mlp_fwd: xln is saved next to hpre only");
            MMG_CHECK_ARG(!a.gact || a.hpre, "mmg_cnblock_mlp_fwd: gact is saved next to hpre only");
            MMG_CHECK_ARG(a.hpre_kind == 0 || (a.hpre_kind == 1 && a.hpre && a.gact),
                          "mmg_cnblock_mlp_fwd: hpre_kind=%d (1 = GELU' in place of the pre-activation) needs hpre and gact", a.hpre_kind);
            return 0;
        case CN_BWD: {
            MMG_CHECK_ARG(a.operands, "mmg_cnblock_mlp_bwd: null pointer");
            const int mode = cn_mlp_bwd_mode(C);
            MMG_CHECK_ARG(mode != 0, "mmg_cnblock_mlp_bwd: C=%d not in {96,128,192,384}", C);
            MMG_CHECK_ARG((mode == 2) == (a.hpre != nullptr), "mmg_cnblock_mlp_bwd: hpre is required for C=384 and unused otherwise (C=%d)", C);
            MMG_CHECK_ARG(M > 0 && M < (1LL << 36), "mmg_cnblock_mlp_bwd: bad M=%lld", M);
            MMG_CHECK_ARG((a.ln_dw == nullptr) == (a.ln_db == nullptr), "mmg_cnblock_mlp_bwd: ln_dw and ln_db go together");
            return 0;
        }
        case CN_BWDW:
            MMG_CHECK_ARG(cn_bwdw_supported(C), "mmg_cnblock_bwdw: C=%d is not supported (96)", C);
            MMG_CHECK_ARG(M > 0 && M % cn_bw_cfg(C).R == 0, "mmg_cnblock_bwdw: M=%lld must be a positive multiple of %d", M, cn_bw_cfg(C).R);
            // M C 2 < 2^32 bytes, written so that no M overflows the product
            MMG_CHECK_ARG(M <= ((1LL << 32) - 1) / (2 * C), "mmg_cnblock_bwdw: M=%lld rows exceed the 4 GiB buffer range of one launch", M);
            MMG_CHECK_ARG(a.operands, "mmg_cnblock_bwdw: null pointer");
            return 0;
        case CN_PACK:
            MMG_CHECK_ARG(a.operands, "mmg_cnblock_pack_weights: null pointer");
            MMG_CHECK_ARG(cn_mlp_supported(C), "mmg_cnblock_pack_weights: C=%d not in {96,128,192,256,384,512}", C);
            MMG_CHECK_ARG(a.backward >= 0 && a.backward <= 2, "mmg_cnblock_pack_weights: backward=%d not in {0,1,2}", a.backward);
            MMG_CHECK_ARG(!a.backward || a.gamma, "mmg_cnblock_pack_weights: the backward image needs the layer scale");
            return 0;
        case CN_BWDW_PACK:
            MMG_CHECK_ARG(cn_bwdw_supported(C), "mmg_cnblock_bwdw_pack: C=%d is not supported (96)", C);
            MMG_CHECK_ARG(a.operands, "mmg_cnblock_bwdw_pack: null pointer");
            return 0;
    }
    mmg_set_error("cn_check: door=%d", door);
    return 1;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
CnPlan cn_plan(int door, long long M, int C, int save, int ln, int cus, const CnKnobs& kn) {
    CnPlan p = {};
    if (door == CN_BWDW) {
        // launch 1's schedule (the kernel's VAR comment).  12 waves (three per SIMD, 168 registers): same-box A/B at 16.8 M rows, two runs each:
        // 13.10 / 13.15 ms against 12.94 / 13.09 with 8 waves - the launch is bound by VALU issue (GELU), not by latency, so the third wave
        // buys nothing.  Off by default; it exists with schedule 0 only.
        const int var = kn.bwdw_var == 2 ? 2 : (kn.bwdw_var == 1 ? 1 : 0);
        p.kernel = kn.bwdw_w12 ? CN_KEY(CN_FAM_bwdw, C, 1, 12, 0) : CN_KEY(CN_FAM_bwdw, C, 1, 8, var);
        p.kernel2 = CN_KEY(CN_FAM_bwdw, C, 2, 8, kn.bwdw_hto ? 1 : 0);
        p.tile = cn_bw_cfg(C).R;
        p.ntiles = (int)(M / p.tile);
        p.grid = p.ntiles < cus ? p.ntiles : cus;           // one persistent workgroup per CU
        p.block = kn.bwdw_w12 ? 768 : 512;
        p.block2 = 512;
        p.lds = cn_bw_cfg(C).LDS;
        return p;
    }
    const CnCfg cfg = cn_cfg(C);
    const int img = 2 * cfg.NC * C * 2;                     // one chunk of the forward: a W1 part and a W2 part, bf16
    const int vectors = 8 * C * (int)sizeof(float);        // ln_w, ln_b [C], b1 [4C], b2, gamma [C] (backward: its own 8C floats)
    p.block = p.block2 = 64 * cfg.WAVES;
    if (door == CN_BWD) {
        const int recomp = cn_mlp_bwd_mode(C) == 1;         // C = 384 reads the forward's saved pre-activation: no W1 part
        p.kernel = CN_KEY(CN_FAM_bwd, C, recomp, ln ? 1 : 0, 0);
        p.tile = cfg.BM;
        p.ntiles = (int)((M + p.tile - 1) / p.tile);
        const int cap = cfg.WGS_BWD * cus;
        p.grid = p.ntiles < cap ? p.ntiles : cap;
        p.lds = 2 * ((recomp ? 3 : 2) * cfg.NC * C * 2) + vectors;
        // The 4C-wide outputs (g, dh) beyond the 256 MiB Infinity Cache are consumed much later by the weight-gradient GEMMs: stored past L2
        // (nontemporal) from C = 128 up.  Same-run A/B (profiles/r02_mlp_nt_store_ab.txt): backward -8...-17 % at C = 192, -12 % at 384, no
        // change at 96; the forward's saved pre-activation is 1-3 % SLOWER that way and keeps plain stores unless the knob forces it
        p.nt = kn.nt_store >= 0 ? kn.nt_store : (C >= 128 && (size_t)M * 4 * C * 2 >= ((size_t)256 << 20));
        return p;
    }
    // resident weights (C = 96 only: both matrices fit the CU's LDS; see the kernel): ONE workgroup of rw waves per CU, each wave walks its
    // own 32-row tiles.  MMG_MLP_FWD_RES = rw (8 / 12; anything else = the streaming form)
    const int rw = (C == 96 && !save && (kn.fwd_res == 8 || kn.fwd_res == 12)) ? kn.fwd_res : 0;
    p.kernel = CN_KEY(CN_FAM_fwd, C, save ? 1 : 0, rw, 0);
    p.nt = save && kn.nt_store >= 0 ? kn.nt_store : 0;
    if (rw) {
        p.tile = 16 * cfg.MT;
        p.ntiles = (int)((M + p.tile - 1) / p.tile);
        const int wgs = (p.ntiles + rw - 1) / rw;
        p.grid = wgs < cus ? wgs : cus;
        p.block = p.block2 = 64 * rw;
        p.lds = (4 * C / cfg.NC) * img + vectors;
        return p;
    }
    p.tile = cfg.BM;
    p.ntiles = (int)((M + p.tile - 1) / p.tile);
    const int cap = cfg.WGS * cus;
    p.grid = p.ntiles < cap ? p.ntiles : cap;
    p.lds = 2 * img + vectors;
    return p;
}

// ---- the read-only door ---------------------------------------------------------------------------------------------------------------------
MMG_API const char* mmg_cnblock_plan(int op, long long M, int C, int save, int ln, int cus) {
    static thread_local char text[192];
    static char dummy[16];                          // stands for the operands: the checks compare pointers with NULL and never dereference
    text[0] = 0;
    if (op < CN_FWD || op > CN_BWDW || cus < 0 || (save && op != CN_FWD) || (ln && op != CN_BWD)) {
        mmg_set_error("mmg_cnblock_plan: op=%d save=%d ln=%d cus=%d (op 0..2; save: op 0; ln: op 1; cus >= 0)", op, save, ln, cus);
        return text;
    }
    CnArgs a = {};
    a.M = M; a.C = C; a.operands = 1;
    if (save) a.hpre = a.mean = a.rstd = dummy;
    if (op == CN_BWD && cn_mlp_bwd_mode(C) == 2) a.hpre = dummy;
    if (ln) a.ln_dw = a.ln_db = dummy;
    if (cn_check(op, a)) return text;
    const CnPlan p = cn_plan(op, M, C, save, ln, cus ? cus : mmg_cu_count_cached(), cn_knobs());
    int n = snprintf(text, sizeof(text), "%s grid=%d ", cn_plan_name(p), p.grid);
    if (p.kernel2) n += snprintf(text + n, sizeof(text) - n, "block=(%d,%d)", p.block, p.block2);
    else n += snprintf(text + n, sizeof(text) - n, "block=%d", p.block);
    snprintf(text + n, sizeof(text) - n, " lds=%d nt=%d tiles=%d", p.lds, p.nt, p.ntiles);
    return text;
}
