// Host-side planning of the five LayerNorm doors (mmg_layernorm_fwd / _fwd_f32 / _fwd_fp8 / _bwd / _bwd_f32): the argument checks, the two
// A/B knobs, and for every launch ONE plan - which kernel instantiation, on how many blocks, with how much LDS, with or without streaming
// stores.  Pure integer arithmetic: no HIP call and no kernel, so the rules are pinned by a CPU test (tests/test_layernorm_plan_cpu.py,
// through the read-only door mmg_layernorm_plan).  norm_elementwise.hip validates, plans, and launches what the plan names.
#pragma once
#include "common.h"

// ---- the kernel instantiations: P(OP, G) = layernorm_OP_plain_kernel<G>, X(OP, G, CH) = layernorm_OP_kernel<G, CH>.  Ids, the names
// mmg_last_kernel() reports and the launch switch of norm_elementwise.hip are all generated from this table: nothing is built that it does
// not list (the backward has no <G, 3>: see ln_plan), and a plan outside it has no name and is refused by the switch. -------------------
#define LN_KERNELS(P, X)                                                                                                            \
    P(fwd, 4) P(fwd, 8) P(fwd, 16) P(fwd, 32) P(fwd, 64) P(bwd, 4) P(bwd, 8) P(bwd, 16) P(bwd, 32) P(bwd, 64)                       \
    X(fwd, 8, 3) X(fwd, 16, 3) X(fwd, 32, 3) X(fwd, 64, 3)                                                                          \
    X(fwd, 8, 1) X(fwd, 16, 1) X(fwd, 32, 1) X(fwd, 64, 1) X(fwd, 64, 2) X(fwd, 64, 4) X(fwd, 64, 8)                                \
    X(bwd, 8, 1) X(bwd, 16, 1) X(bwd, 32, 1) X(bwd, 64, 1) X(bwd, 64, 2) X(bwd, 64, 4) X(bwd, 64, 8)

enum { LN_OP_fwd = 0, LN_OP_bwd = 1 };
#define LN_KEY(BWD, PLAIN, G, CH) ((((BWD) * 2 + (PLAIN)) * 128 + (G)) * 16 + (CH))      // an id is its instantiation, packed (never 0)
enum LNKernel {
#define P(OP, G) LK_##OP##_plain_##G = LN_KEY(LN_OP_##OP, 1, G, 3),
#define X(OP, G, CH) LK_##OP##_##G##_##CH = LN_KEY(LN_OP_##OP, 0, G, CH),
    LN_KERNELS(P, X)
#undef P
#undef X
};
const char* ln_kernel_name(int kernel);        // as rocprofv3's kernel trace spells it: "layernorm_bwd_kernel<64, 2>"; "" when not in the table

// ---- the doors ------------------------------------------------------------------------------------------------------------------------------
enum LNDoorId { LN_FWD = 0, LN_FWD_F32 = 1, LN_FWD_FP8 = 2, LN_BWD = 3, LN_BWD_F32 = 4, LN_DOORS = 5 };   // = door of mmg_layernorm_plan
struct LNDoor {
    const char* name;       // "mmg_layernorm_fwd" ...
    int bwd;
    int x_f32, y_fp8;       // LNArgs::x_f32 / y_fp8 of every launch through this door
    int nt;                 // the streaming stores apply (ln_plan)
};
const LNDoor& ln_door(int door);

// ---- tuning knobs (A/B switches, tools/ln_ab.py).  Read on EVERY call: tests and that tool set them inside one process. -----------------
struct LNKnobs {
    int plain;              // MMG_LN_PLAIN   1      0: the image tower's widths stay on the generic templates
    int ch3;                // MMG_LN_CH3     1      0: no three-chunk rows in the generic forward
};
LNKnobs ln_knobs();

// ---- what the kernels receive (by value: the layout is part of the device code) -------------------------------------------------------------
struct LNArgs {
    const bf16_t* x; int ldx;
    const float* gamma; const float* beta; float eps;
    bf16_t* y; int ldy;
    float* mean; float* rstd;
    int M, C;
    int patch, H, W;     // patchified output (H, W = spatial dims of the INPUT rows)
    // backward
    const bf16_t* dy; int lddy;
    bf16_t* dx; int lddx;
    float* dgamma; float* dbeta;
    const bf16_t* add; int ldadd;    // optional residual-path gradient added to dx (pre-LN transformer blocks)
    int nt;                          // stream the output past L2 (tensor larger than the Infinity Cache)
    int y_fp8;                       // y receives OCP e4m3 bytes (ldy in bytes): operand of the fp8 GEMM path
    int x_f32;                       // x holds fp32 (the text tower keeps its pre-LayerNorm sums in fp32); ldx in elements
    float* yf; int ldyf;             // optional fp32 copy of y (the text tower's residual stream), forward only
    const float* res; int ldres;     // optional fp32 residual: the row normalised is x + res, and x is OVERWRITTEN with that sum
};

// ---- one validated argument path: non-zero = rejected, the message (mmg_last_error) starts with the door's name.  Reads the operands,
// leading dimensions and shape of `a` (a door leaves what it does not take at zero); nt / y_fp8 / x_f32 are not inputs. -------------------
int ln_check(int door, const LNArgs& a);

// ---- one plan per launch ------------------------------------------------------------------------------------------------------------------
struct LNPlan {
    int kernel;                     // LNKernel = LN_KEY(backward, plain template, G, CH)
    int G, CH;                      // lanes per row, 16-byte chunks per lane
    int rows_per_block;             // 4 waves x 64 / G rows
    int blocks, block, lds;         // grid, block size, dynamic LDS bytes
    int nt;                         // LNArgs::nt
};
// res / yf / add: the call has that optional operand
LNPlan ln_plan(int door, int M, int C, int res, int yf, int add, const LNKnobs& kn);
