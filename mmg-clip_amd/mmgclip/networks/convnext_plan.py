"""Which kernels a CNBlock of the ConvNeXt tower runs through - decided here, once, as plain values (no tensors, no device).

Three decisions, each made where everything it needs is known, each a record that is handed on instead of being inferred again:
  * `BlockPlan`     per tower and width, when the working copies are built: which forward / backward forms exist for this block;
  * `SaveDecision`  per recorded forward: which optional tensors that forward keeps for its backward (they have to fit the device);
  * `BlockSaved`    per block and micro-batch: what the forward kept and which backward form reads it (`saving_form`).
The table of DESIGN.md section 3 ("Which path a CNBlock takes") is these functions' output; tests/test_convnext_plan_cpu.py holds them to it.
"""
from typing import Any, Callable, NamedTuple, Optional

from .. import kernels as K


class Support(NamedTuple):
    """What the kernel library offers at a width: the planner's only questions to it (tests pass their own answers)."""
    fused_fwd: Callable[[int], bool] = K.cnblock_supported            # mmg_cnblock_mlp_fwd exists for C
    fused_bwd_mode: Callable[[int], int] = K.cnblock_bwd_mode         # mmg_cnblock_mlp_bwd: 0 no, 1 recomputes the hidden row, 2 reads the saved one
    bwdw: Callable[[int, int], bool] = K.cnblock_bwdw_supported       # mmg_cnblock_bwdw runs C at M rows


class Knobs(NamedTuple):
    """The tower's settings the plan depends on (ConvNextTower.__init__ reads them from its arguments and the MMG_* environment)."""
    fp8: bool = False
    fp8_min_channels: int = 256
    fp8_bwd: bool = True                # MMG_FP8_BWD != 0
    fused_mlp: bool = True              # MMG_FUSED_MLP != 0
    fused_bwd_saved_h: bool = False     # MMG_FUSED_MLP_BWD_SAVED_H == 1
    bwdw: bool = True                   # MMG_BWDW != 0
    fused_save_maxc: int = 384          # MMG_MLP_FUSED_SAVE_MAXC


class BlockPlan(NamedTuple):
    C: int
    kind: str                   # forward MLP: "fp8" (GEMM pair on e4m3 operands), "fused" (one launch), "gemm" (GEMM pair, bf16)
    fused_bwd: int              # the fused backward at this width: 0 none (GEMM pair), 1 recomputes the hidden row, 2 reads the saved one
    bwdw: bool                  # fused_bwd == 1 and the weight gradients can be accumulated on chip (csrc/cnblock_bwdw.hip; row count permitting)
    fp8_bwd_weights: bool       # an fp8 block that holds the e4m3 weights of the 8-bit backward
    fused_save_maxc: int        # widest "fused" block whose SAVING forward stays on the fused kernel (beyond it: only when nothing is saved)


class SaveDecision(NamedTuple):
    save_ln: bool               # GEMM-pair backwards get the LayerNorm output ([M,C] bf16) from the forward instead of recomputing it
    save_gelu: bool             # ... and GELU(hidden) ([M,4C] bf16): their data-gradient GEMM then applies GELU' only
    fp8_bwd_now: bool           # fp8 blocks keep their e4m3 operands and run the 8-bit backward (otherwise: the bf16 one on the saved hidden)


class BlockSaved(NamedTuple):
    """What one block's forward kept for one micro-batch."""
    x: Any                      # block input [M,C] bf16
    d: Any                      # depthwise output [M,C] bf16
    mean: Any                   # LayerNorm statistics fp32 [M] (None where the backward recomputes them)
    rstd: Any
    aux: Any                    # the 4C-wide bf16 tensor, see aux_kind
    aux_kind: Optional[str]     # None (nothing 4C-wide kept), "h" (pre-GELU hidden) or "dgelu" (GELU'(hidden))
    ln: Any                     # LayerNorm output: bf16 (save_ln), e4m3 bytes (bwd == "fp8") or None (rebuilt)
    g: Any                      # GELU(hidden): bf16 (save_gelu), e4m3 bytes (bwd == "fp8") or None (rebuilt)
    bwd: str                    # "bwdw", "fused", "fp8" or "gemm": ConvNextTower._bwd_<bwd>


def plan_block(C, knobs, support=Support()):
    if knobs.fp8 and C % 128 == 0 and C >= knobs.fp8_min_channels:
        kind = "fp8"
    elif knobs.fused_mlp and support.fused_fwd(C):
        kind = "fused"
    else:
        kind = "gemm"
    mode = support.fused_bwd_mode(C)
    if mode == 2 and not knobs.fused_bwd_saved_h:         # (C = 384: slower than the GEMM pair so far)
        mode = 0
    return BlockPlan(C, kind, mode, mode == 1 and knobs.bwdw and support.bwdw(C, 64), kind == "fp8" and knobs.fp8_bwd, knobs.fused_save_maxc)


def fused_forward(p, save):
    """LN + Linear + GELU + Linear + layer scale + residual in one launch?  (C = 512, ConvNeXt-B stage 3: only when nothing is saved for a
    backward - with the 4C-wide store it is no faster than the GEMM pair; at C = 384 it stores three 4C- / C-wide streams beside its output
    and the GEMM pair is within reach of it, hence the A/B knob)"""
    return p.kind == "fused" and (not save or p.C <= p.fused_save_maxc)


def saving_form(p, dec, M, save_dgelu=True, support=Support()):
    """What a saving forward over M rows keeps, and for which backward: -> (BlockSaved.bwd, BlockSaved.aux_kind, keep .ln, keep .g).
    save_dgelu: with GELU(hidden) kept, the second 4C-wide tensor is GELU'(hidden) instead of the hidden itself (same bytes): the backward's
    data-gradient GEMM then multiplies by it instead of evaluating the polynomial per element (MMG_SAVE_DGELU=0: the hidden)."""
    if p.kind == "fp8":
        # 8-bit backward: GELU'(h) - its data-gradient GEMM multiplies by it - and the e4m3 LayerNorm output / activation, which ARE the
        # weight-gradient GEMMs' operands.  They are not what the bf16 backward reads: that one keeps h and rebuilds both
        return ("fp8", "dgelu", True, True) if (p.fp8_bwd_weights and dec.fp8_bwd_now) else ("gemm", "h", False, False)
    if fused_forward(p, True) and p.fused_bwd:
        bwd = "bwdw" if (p.bwdw and support.bwdw(p.C, M)) else "fused"
        return bwd, (None if p.fused_bwd == 1 else "h"), False, False           # (mode 1 recomputes the hidden row on chip)
    return "gemm", ("dgelu" if (dec.save_gelu and save_dgelu) else "h"), dec.save_ln, dec.save_gelu


def decide_saves(plan, depths, alive, total_memory, ckpt=False, save_ln="auto", save_gelu="auto", fp8_bwd="0"):
    """plan, depths: one BlockPlan and block count per stage.  alive: (n, H, W) triples - images whose saved tensors are alive at once (the
    whole batch; one micro-batch under checkpointing; one triple per image size).  The three modes (MMG_SAVE_LN, MMG_SAVE_GELU,
    MMG_FP8_BWD; fp8_bwd is "0" for a tower without fp8): "0" off, "1" on, anything else by memory - the optional copies are kept while they stay below a share of the device:
      LayerNorm outputs of the GEMM-pair backwards ([M,C] bf16)            4 %   (C2: 8.4 GB, on; ConvNeXt-B at 256 images: 31 GB beside 267 GiB, off)
      their GELU(hidden) ([M,4C] bf16)                                    15 %   (C2: 33.8 GB, on; ConvNeXt-B: 131 GB, off)
      e4m3 LayerNorm output + activation of the fp8 blocks (5 C bytes)    15 %   (C5, micro-batches of 64: 23 GB, on; ConvNeXt-B at 256 images: 93 GB, off)
    ckpt: under checkpointing the saved tensors of ONE micro-batch are all the activation memory there is, so they may take a larger share
    (10 / 30 / 20 %; ConvNeXt-B in micro-batches of 128: 264 against 249 pairs/s with them, peak 238 GiB)."""
    extra = keep8 = 0
    for n, H, W in alive:
        hh, ww = H // 4, W // 4
        for p, depth in zip(plan, depths):
            if not p.fused_bwd:
                extra += depth * n * hh * ww * p.C * 2
            if p.fp8_bwd_weights:
                keep8 += depth * n * hh * ww * p.C * 5
            hh, ww = hh // 2, ww // 2
    return SaveDecision(
        save_ln == "1" if save_ln in ("0", "1") else extra <= (0.10 if ckpt else 0.04) * total_memory,
        save_gelu == "1" if save_gelu in ("0", "1") else 4 * extra <= (0.30 if ckpt else 0.15) * total_memory,       # ([M,4C] against [M,C])
        fp8_bwd != "0" and (fp8_bwd == "1" or keep8 <= (0.20 if ckpt else 0.15) * total_memory))
