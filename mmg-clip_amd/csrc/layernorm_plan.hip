// Host-only half of the LayerNorm doors (see layernorm_plan.h): knobs, argument checks, kernel selection, grid and LDS size, and the
// read-only door mmg_layernorm_plan.  No device call, no kernel: what a launch will be is decided here and can be asked for without launching.
#include "layernorm_plan.h"
#include <stdlib.h>

// ---- kernel table ---------------------------------------------------------------------------------------------------------------------------
const char* ln_kernel_name(int kernel) {
    switch (kernel) {
#define P(OP, G) case LK_##OP##_plain_##G: return "layernorm_" #OP "_plain_kernel<" #G ">";
#define X(OP, G, CH) case LK_##OP##_##G##_##CH: return "layernorm_" #OP "_kernel<" #G ", " #CH ">";
        LN_KERNELS(P, X)
#undef P
#undef X
    }
    return "";
}

// ---- doors and knobs ------------------------------------------------------------------------------------------------------------------------
// {name, bwd, x_f32, y_fp8, nt}.  nt: the two bf16-row doors stream an output larger than the 256 MiB Infinity Cache past L2 (ln_plan); the
// fp32-row doors and the fp8 door never have (nothing was measured for them), and keep their plain stores at every size
static const LNDoor kDoors[LN_DOORS] = {
    {"mmg_layernorm_fwd", 0, 0, 0, 1},     {"mmg_layernorm_fwd_f32", 0, 1, 0, 0}, {"mmg_layernorm_fwd_fp8", 0, 0, 1, 0},
    {"mmg_layernorm_bwd", 1, 0, 0, 1},     {"mmg_layernorm_bwd_f32", 1, 1, 0, 0},
};
const LNDoor& ln_door(int door) { return kDoors[door]; }

static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
LNKnobs ln_knobs() { return {env_int("MMG_LN_PLAIN", 1), env_int("MMG_LN_CH3", 1)}; }

// ---- argument checks --------------------------------------------------------------------------------------------------------------------------
int ln_check(int door, const LNArgs& a) {
    const LNDoor& d = ln_door(door);
    const char* n = d.name;
    const int M = a.M, C = a.C;
    MMG_CHECK_ARG(M > 0 && C >= 8 && C % 8 == 0 && C <= 4096, "%s: M=%d C=%d (C must be a multiple of 8, <= 4096)", n, M, C);
    MMG_CHECK_ARG(!a.patch || (a.H > 1 && a.W > 1 && M % (a.H * a.W) == 0), "%s: patchified layout needs H=%d W=%d dividing M=%d", n, a.H, a.W, M);
    const int out_min = a.patch ? 4 * C : C;        // y / dy: a patchified row holds the four pixels of its 2 x 2 patch (fp8 y: ldy in bytes)
    if (!d.bwd) {
        MMG_CHECK_ARG(a.x && a.gamma && a.beta && a.y && a.ldx % 8 == 0 && a.ldy % 8 == 0 && a.ldx >= C && a.ldy >= out_min &&
                          (!a.yf || (a.ldyf >= C && a.ldyf % 4 == 0)) && (!a.res || (a.ldres >= C && a.ldres % 4 == 0)),
                      "%s: bad pointer or leading dimension", n);
        return 0;
    }
    // odd H / W: dy is [(M / (H W)) (H/2) (W/2), 4C] as the forward wrote it; the dropped pixels get dx = 0 (+ add) and no dy address is formed
    MMG_CHECK_ARG(a.dy && a.x && a.mean && a.rstd && a.gamma && a.dx && ((a.dgamma == nullptr) == (a.dbeta == nullptr)) && a.ldx % 8 == 0 &&
                      a.lddy % 8 == 0 && a.lddx % 8 == 0 && a.ldx >= C && a.lddx >= C && a.lddy >= out_min,
                  "%s: bad pointer or leading dimension", n);
    MMG_CHECK_ARG(!a.add || (a.ldadd >= C && a.ldadd % 8 == 0), "%s: bad ldadd=%d", n, a.ldadd);
    return 0;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
LNPlan ln_plan(int door, int M, int C, int res, int yf, int add, const LNKnobs& kn) {
    const LNDoor& d = ln_door(door);
    // a row is owned by a group of G lanes (power of two >= C / 8, 8 ... 64), CH 16-byte chunks per lane (1, 2, 4, 8: C <= 4096)
    const int nch = C / 8;
    int G = 8;
    while (G < nch && G < 64) G <<= 1;
    const int ch = cdiv(nch, G);
    int CH = ch <= 1 ? 1 : ch <= 2 ? 2 : ch <= 4 ? 4 : 8;
    const int g3 = nch % 3 == 0 ? nch / 3 : 0;
    const bool g3_pow2 = g3 == 8 || g3 == 16 || g3 == 32 || g3 == 64;
    // round 3, FORWARD only: widths of 3 x 2^k chunks (192, 384, 768, 1536: every ConvNeXt-T / BERT width but 96) take G = 2^k lanes x 3
    // chunks per row instead of the next power of two with a quarter of the lanes idle: no idle lanes, 64 / G rows and three times the bytes
    // in flight per wave.  Same-run A/B (tools/ln_ab.py, profiles/r03_ln_ab.txt): forward 498 -> 389 us at M = 1 M x 384 (3.2 -> 4.1 TB/s),
    // 213 -> 191 at 262 k x 768, 779 -> 745 at 4.2 M x 192; the BACKWARD got slower with it (652 -> 805, 1231 -> 1523, 321 -> 432 us: three
    // chunks of dgamma / dbeta accumulators and operands per lane) and keeps the round-2 selection.  MMG_LN_CH3=0: off (A/B).
    if (!d.bwd && kn.ch3 && g3_pow2) { G = g3; CH = 3; }
    // the image tower's widths on the plain templates, which have no fp32-row / residual / fp32-copy / fp8 / add variants (MMG_LN_PLAIN=0: off, A/B)
    const bool plain = kn.plain && (g3 == 4 || g3_pow2) && !d.x_f32 && !res && !d.y_fp8 && !yf && !add;
    if (plain) { G = g3; CH = 3; }
    LNPlan p = {};
    p.kernel = LN_KEY(d.bwd, plain ? 1 : 0, G, CH);
    p.G = G;
    p.CH = CH;
    p.rows_per_block = 4 * (64 / G);
    p.blocks = cdiv(M, p.rows_per_block);
    const int cap = d.bwd ? 1024 : 4096;            // the rows beyond go round the kernels' grid-stride loop
    if (p.blocks > cap) p.blocks = cap;
    p.block = 256;
    p.lds = d.bwd ? 2 * C * (int)sizeof(float) : 0; // the block's dgamma / dbeta partial sums
    p.nt = d.nt && (size_t)M * C * 2 >= ((size_t)256 << 20);
    return p;
}

// ---- the read-only door ---------------------------------------------------------------------------------------------------------------------
MMG_API const char* mmg_layernorm_plan(int door, int M, int C, int res, int yf, int add) {
    static thread_local char text[128];
    static char dummy[16];                          // stands for the operands: the checks compare pointers with NULL and never dereference
    text[0] = 0;
    if (door < 0 || door >= LN_DOORS || ((res || yf) && door != LN_FWD_F32) || (add && !ln_door(door).bwd)) {
        mmg_set_error("mmg_layernorm_plan: door=%d res=%d yf=%d add=%d (door 0..4; res, yf: door 1; add: doors 3, 4)", door, res, yf, add);
        return text;
    }
    LNArgs a = {};
    a.M = M; a.C = C;
    a.x = a.dy = a.add = (const bf16_t*)dummy; a.y = a.dx = (bf16_t*)dummy;
    a.gamma = a.beta = a.res = (const float*)dummy; a.mean = a.rstd = a.yf = (float*)dummy;
    a.ldx = a.ldy = a.lddy = a.lddx = a.ldadd = a.ldyf = a.ldres = C;
    if (!res) a.res = nullptr;
    if (!yf) a.yf = nullptr;
    if (!add) a.add = nullptr;
    if (ln_check(door, a)) return text;
    const LNPlan p = ln_plan(door, M, C, res, yf, add, ln_knobs());
    snprintf(text, sizeof(text), "%s grid=%d block=%d lds=%d nt=%d", ln_kernel_name(p.kernel), p.blocks, p.block, p.lds, p.nt);
    return text;
}
