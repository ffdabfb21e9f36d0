"""ConvNeXt image tower on the HIP kernels: forward + backward over NHWC bf16 activations.

What the reference has (path:line in the reference tree): `ConvNextTiny.forward` = `model.features(x)` then
`model.avgpool(x)` on a torchvision-layout ConvNeXt-T TorchScript archive (mmgclip/networks/encoder.py:40-55), fed by
`(x*65535 - 32767.5)/32767.5` (mmgclip/networks/image_features.py:95-99); module tree printed in
notebooks/clf_convnext_tiny_experimental.ipynb cell 3 (Conv2dNormActivation(Conv2d 4x4/4, LayerNorm2d), CNBlock(dwconv7,
Permute, LayerNorm, Linear C->4C, GELU, Linear 4C->C, Permute) * layer_scale + residual, depths 3/3/9/3, dims
96/192/384/768; downsample = LayerNorm2d + Conv2d 2x2/2).  The reference never trains it; the backward here is new
capability (north star) and is checked against oracle/encoders_oracle.py.

Parameter names/shapes follow torchvision (`features.{i}.{j}.block.{k}.weight`, `layer_scale` ...) so a torchvision
state dict loads unchanged.  Stochastic depth (torchvision's `StochasticDepth(p, "row")` at the end of every CNBlock) is off by default
(`stochastic_depth_prob=0`); with a rate, a training-mode forward drops whole samples per block and never computes them: the schedule
is convnext_sd.py's, the image moves are csrc/stochastic_depth.hip's.

Data layout on the MI355X: activations are bf16 [n*H*W, C] (NHWC flattened), so every pointwise Linear is a plain
row-major GEMM and LayerNorm reads contiguous rows; the 2x2/4x4 stride=kernel convolutions become GEMMs on patchified
rows (the LayerNorm kernel writes the patchified layout directly).  Blocks with C <= 384 run LayerNorm + Linear + GELU +
Linear + layer scale + residual as one fused launch (csrc/cnblock_mlp.hip); for C <= 192 the backward recomputes the hidden
row on chip.  Saved for backward per block and pixel: block input (C), depthwise output (C) and - only where the backward
does not recompute it - the pre-GELU hidden (4C) in bf16 + LN statistics; LN output and GELU output are rebuilt, or kept while they fit.
Which form a block takes, and what it keeps, is decided in convnext_plan.py (table: DESIGN.md section 3).

Image sizes: any H, W >= 32, forward and backward.  Every strided layer floors (stem H // 4, downsample // 2) and drops the odd last row /
column as torch's convolutions do; the forward records each stage's map size and the backward reads it back (dropped pixels get a zero
gradient from mmg_layernorm_bwd).  `forward` also takes a list of [Cin, H_i, W_i] images of different sizes: grouped by size in order of first
appearance (`group_by_size`), each group in micro-batches of its own, features and gradients routed back in input order.
"""
import ctypes
import os

import torch
import torch.nn as nn

from .. import _hip
from .. import kernels as K
from .. import linalg as L
from .._hip import call, ptr, stream
from ..params import backward_finished, last_backward
from . import convnext_sd as SD
from .convnext_plan import BlockSaved, Knobs, decide_saves, fused_forward, plan_block, saving_form
from .tower import Tower, as_pixels, augment_tables, backward_parts, conv_weight_rows, fold_conv_grad, forward_parts

CONFIGS = {
    "tiny": dict(depths=(3, 3, 9, 3), dims=(96, 192, 384, 768)),
    "small": dict(depths=(3, 3, 27, 3), dims=(96, 192, 384, 768)),
    "base": dict(depths=(3, 3, 27, 3), dims=(128, 256, 512, 1024)),
}
LN_EPS = 1e-6


def _fused_save_maxc():
    """MMG_MLP_FUSED_SAVE_MAXC (A/B knob, round 4; BlockPlan.fused_save_maxc).  Read per forward: tools/ flip it within a process."""
    return int(os.environ.get("MMG_MLP_FUSED_SAVE_MAXC", "384"))


def lnbwd_fused(M, N, Kd, C, patch_hw=None):
    """Whether the data-gradient GEMM [M,Kd] x [N,Kd]^T in front of a LayerNorm backward of width C takes the one-launch form
    (csrc/gemm_lnbwd.hip): MMG_LNBWD_FUSED != 0 (read per call) and a shape the kernel has."""
    return K.lnbwd_fused_enabled() and K.gemm_nt_lnbwd_supported(N, Kd, C, patch_hw)


class LayerNorm2d(nn.LayerNorm):
    """Parameter container with torchvision's name; the arithmetic runs in mmg_layernorm_fwd."""


class CNBlock(nn.Module):
    def __init__(self, dim, layer_scale=1e-6):
        super().__init__()
        self.block = nn.Sequential(
            nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim, bias=True),
            nn.Identity(),                      # Permute([0, 2, 3, 1])
            nn.LayerNorm(dim, eps=LN_EPS),
            nn.Linear(dim, 4 * dim, bias=True),
            nn.GELU(),
            nn.Linear(4 * dim, dim, bias=True),
            nn.Identity(),                      # Permute([0, 3, 1, 2])
        )
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * layer_scale)


def build_features(variant="tiny", in_chans=1):
    cfg = CONFIGS[variant]
    dims, depths = cfg["dims"], cfg["depths"]
    layers = [nn.Sequential(nn.Conv2d(in_chans, dims[0], kernel_size=4, stride=4, bias=True), LayerNorm2d(dims[0], eps=LN_EPS))]
    for i, (d, n) in enumerate(zip(dims, depths)):
        layers.append(nn.Sequential(*[CNBlock(d) for _ in range(n)]))
        if i < 3:
            layers.append(nn.Sequential(LayerNorm2d(d, eps=LN_EPS), nn.Conv2d(d, dims[i + 1], kernel_size=2, stride=2)))
    feats = nn.Sequential(*layers)
    for m in feats.modules():                       # torchvision ConvNeXt init
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
    return feats


class _TorchvisionLayout(nn.Module):
    """`.features` / `.avgpool` holder so state-dict keys read `model.features...` like the reference archive."""

    def __init__(self, variant, in_chans):
        super().__init__()
        self.features = build_features(variant, in_chans)
        self.avgpool = nn.AdaptiveAvgPool2d(1)


class ConvNextTower(Tower):
    """pixels [n, Cin, H, W], fp32 in [0,1] or raw uint16 / uint8 (scale16=True applies the reference's 16-bit scaling) -> features
    [n, dims[-1]].  augment (None | AugmentSpec | mapping, mmgclip/augment.py): seeded flip / shift / tone inside the stem's patchify, in
    training mode only."""

    def __init__(self, variant="tiny", in_chans=1, scale16=True, micro_batch=64, fused_mlp=None, checkpoint=False, fp8=False,
                 fp8_min_channels=None, stochastic_depth_prob=0.0, augment=None):
        super().__init__()
        self.set_augment(augment)
        # torchvision's recipes: 0.1 (tiny), 0.4 (small), 0.5 (base); block b of B drops a sample with p_b = rate * b / (B - 1).  Acts in
        # training mode only, with or without gradients; 0 is the path without it, bit for bit
        self.stochastic_depth_prob = SD.check_rate(stochastic_depth_prob)
        self.next_drop_seed = None          # tests: force the seed of the next forward that applies stochastic depth
        self._drop_seeds = SD.DropSeeds()
        self.variant, self.in_chans, self.scale16, self.micro_batch = variant, in_chans, scale16, micro_batch
        # narrow stages (C <= 256) run the CNBlock MLP as one fused launch; MMG_FUSED_MLP=0 keeps the GEMM pair
        self.fused_mlp = (os.environ.get("MMG_FUSED_MLP", "1") != "0") if fused_mlp is None else bool(fused_mlp)
        self.fused_bwd_saved_h = os.environ.get("MMG_FUSED_MLP_BWD_SAVED_H", "0") == "1"
        self.bwdw = os.environ.get("MMG_BWDW", "1") != "0"        # on-chip weight-gradient backward where supported (csrc/cnblock_bwdw.hip)
        # blocks whose backward is the GEMM pair keep their LayerNorm output ([M,C] bf16) instead of recomputing it, and GELU(hidden)
        # ([M,4C] bf16), so that the backward's data-gradient GEMM applies GELU' only (its epilogue is VALU-bound and half of it rebuilt that
        # activation) - decided per forward, while those copies fit the device (convnext_plan.decide_saves).  MMG_SAVE_LN / MMG_SAVE_GELU
        # = 0 / 1 force them.  save_ln, save_gelu (and fp8_bwd_now below) show what the latest recorded forward decided.
        self.save_ln_mode = os.environ.get("MMG_SAVE_LN", "auto")
        self.save_ln = self.save_ln_mode == "1"
        self.save_gelu_mode = os.environ.get("MMG_SAVE_GELU", "auto")
        self.save_gelu = self.save_gelu_mode == "1"
        # with GELU(h) kept, keep GELU'(h) instead of h as the second 4C-wide tensor (round 4; MMG_SAVE_DGELU=0: h, and the polynomial in the backward)
        self.save_dgelu = os.environ.get("MMG_SAVE_DGELU", "1") != "0"
        self.checkpoint = checkpoint        # recompute each micro-batch's forward in the backward (north-star config C5)
        # fp8 (config C5): the two pointwise GEMMs of every block with C % 128 == 0 and C >= fp8_min_channels run their FORWARD
        # on e4m3 operands (LayerNorm / GELU outputs cast unscaled, weights with a per-tensor power-of-two scale); the backward
        # stays bf16 on the saved pre-activation.  Default 512: the stages whose blocks are GEMM pairs anyway.
        self.fp8 = bool(fp8)
        # round 4: the same blocks' BACKWARD in 8 bits too (MMG_FP8_BWD=0: the bf16 backward of rounds 1 - 3): the incoming gradient is cast to e5m2
        # with a per-tensor power-of-two scale, both data-gradient GEMMs run on e5m2 x e4m3 operands (dh handed on in e5m2, written once), both
        # weight-gradient GEMMs on the 8-bit operands the forward / data path already hold (csrc/gemm_tn_fp8.hip)
        # MMG_FP8_BWD: 0 off, 1 always, otherwise (the default) decided per forward - the 8-bit operands are kept only while they fit
        self.fp8_bwd_mode = os.environ.get("MMG_FP8_BWD", "auto")
        self.fp8_bwd = self.fp8_bwd_mode != "0"
        self.fp8_bwd_now = False
        self.fp8_delayed = os.environ.get("MMG_FP8_DELAYED", "1") != "0"      # gradient scale from the previous quantisation of the same tensor role
        self._e5m2_state = {}
        # (round 4, with the 8-bit backward: 256 - same-box A/B of `bench.py --variant base --fp8 --checkpoint`: 925 ms/step from C = 256, 939 from 512,
        #  936 from 128: at C = 256 the GEMM pair's 4C-wide tensors are 8-bit in both directions now; rounds 1 - 3, forward only: no difference, 512)
        self.fp8_min_channels = int(os.environ.get("MMG_FP8_MIN_C", "256" if self.fp8_bwd else "512")) if fp8_min_channels is None else int(fp8_min_channels)
        self.dims, self.depths = CONFIGS[variant]["dims"], CONFIGS[variant]["depths"]
        self.model = _TorchvisionLayout(variant, in_chans)
        self.model_output_dimension = self.dims[-1]
        self.kp = (16 * in_chans + 31) // 32 * 32          # stem GEMM K padded to the MFMA k-step
        self.plan = None                    # one BlockPlan per stage; made with the working copies (knobs may be set after construction)

    # ---- parameter plumbing ------------------------------------------------------------------------------
    def _bound(self):
        self._pname = {id(m): "features." + n for n, m in self.model.features.named_modules()}

    def _g(self, mod, leaf):
        """Gradient view (arena) of parameter `leaf` of module `mod`."""
        return self._arena.g(self._pname[id(mod)] + "." + leaf)

    def stochastic_depth_active(self):
        return self.training and self.stochastic_depth_prob > 0.0

    def reseed_stochastic_depth(self, seed=None):
        """Restart the tower's private seed stream from (seed, rank); seed=None: the last `seeding()` call's seed (convnext_sd.DropSeeds)."""
        self._drop_seeds.reseed(seed)

    def _working_copy_key(self):
        """(+ whether stochastic depth acts, and at which rate: the copies that bake the layer scale in hold gamma / (1 - p_b) then, and
        eval() after train() must not read those)"""
        active = self.stochastic_depth_active()
        return self._arena.version(), active, self.stochastic_depth_prob if active else 0.0

    def knobs(self):
        return Knobs(self.fp8, self.fp8_min_channels, self.fp8_bwd, self.fused_mlp, self.fused_bwd_saved_h, self.bwdw, _fused_save_maxc())

    def _plan_blocks(self):
        return tuple(plan_block(C, self.knobs()) for C in self.dims)

    def _build_working_copies(self):
        """bf16 / transposed / tap-major copies the kernels read.  Which copies a block gets follows from its BlockPlan (self.plan, made
        here)."""
        f = self.model.features
        plan = self.plan = self._plan_blocks()
        wc = {"stem.w": K.cast_bf16(conv_weight_rows(f[0][0].weight.data))}          # [C0, Cin, 4, 4] -> [C0, kp]
        # stochastic depth: a kept sample's branch is scaled by s_b = 1 / (1 - p_b), the same for every kept sample of block b, so the
        # kernels simply read gamma * s_b as their layer scale (".gamma": the vector the forward passes, baked into .w2gt / .w2gt8 /
        # .mlpb / .bwdw below); None: stochastic depth does not act and ".gamma" is the parameter itself
        scales = wc["sd.scales"] = SD.scales(self.stochastic_depth_prob, self.depths) if self.stochastic_depth_active() else None
        b = 0
        for si, p in enumerate(plan):
            C = p.C
            for bi, blk in enumerate(f[1 + 2 * si]):
                key = f"{si}.{bi}"
                w1, w2, gamma = blk.block[3].weight.data, blk.block[5].weight.data, blk.layer_scale.data.reshape(C)
                if scales is not None and scales[b] != 1.0:
                    gamma = gamma * scales[b]
                wc[key + ".gamma"] = gamma
                b += 1
                wc[key + ".w49"] = blk.block[0].weight.data.reshape(C, 49).t().contiguous()
                wc[key + ".w1"] = K.cast_bf16(w1)                                            # [4C, C]
                wc[key + ".w1t"] = K.transpose_cast_bf16(w1)                                 # [C, 4C]
                wc[key + ".w2"] = K.cast_bf16(w2)                                            # [C, 4C]
                wc[key + ".w2gt"] = K.transpose_cast_bf16(w2, gamma)                         # [4C, C] * gamma
                if p.kind == "fp8":                                                          # e4m3 bytes + (scale, 1/scale)
                    wc[key + ".w1f8"], wc[key + ".s1"] = K.quantize_e4m3(w1)
                    wc[key + ".w2f8"], wc[key + ".s2"] = K.quantize_e4m3(w2)
                    if p.fp8_bwd_weights:    # the data-gradient GEMMs' weights: (gamma W2)^T [4C, C] and W1^T [C, 4C], e4m3 + (scale, 1/scale)
                        wc[key + ".w2gt8"], wc[key + ".s2gt"] = K.quantize_e4m3((w2 * gamma.reshape(C, 1)).t().contiguous())
                        wc[key + ".w1t8"], wc[key + ".s1t"] = K.quantize_e4m3(w1.t().contiguous())
                elif p.kind == "fused":                                                      # packed LDS images
                    wc[key + ".mlp"] = K.cnblock_pack(w1, w2)
                    if p.fused_bwd:
                        wc[key + ".mlpb"] = K.cnblock_pack(w1, w2, gamma, backward=p.fused_bwd)
                    if p.bwdw:               # round 3: backward with the weight gradients accumulated on chip (C = 96: nothing 4C-wide reaches HBM)
                        wc[key + ".bwdw"] = K.cnblock_bwdw_pack(w1, w2, blk.block[2].weight.data, blk.block[2].bias.data, gamma,
                                                                blk.block[3].bias.data)
            if si < 3:
                wds = conv_weight_rows(f[2 + 2 * si][1].weight.data)                         # [2C, C, 2, 2] -> [2C, 4C]: no padding
                wc[f"ds{si}.w"] = K.cast_bf16(wds)
                wc[f"ds{si}.wt"] = K.transpose_cast_bf16(wds)
        return wc

    def _decide_saves(self, n_alive, H, W, device, ckpt=False, more=()):
        """-> SaveDecision of a forward whose saved tensors of n_alive H x W images (and of `more`: further (n, H, W) triples, a batch of several
        image sizes) are alive at once; ckpt: they are one checkpointed micro-batch's.  (A tower that has not run yet is planned as it stands.)"""
        return decide_saves(self.plan or self._plan_blocks(), self.depths, ((n_alive, H, W),) + tuple(more),
                            torch.cuda.get_device_properties(device).total_memory, ckpt, self.save_ln_mode, self.save_gelu_mode,
                            self.fp8_bwd_mode if self.fp8 else "0")

    # ---- one block's MLP, forward: -> (block output, BlockSaved or None) ---------------------------------------
    def _saving(self, p, dec, M):
        return saving_form(p, dec, M, self.save_dgelu) if dec is not None else (None, None, False, False)

    def _fwd_fused(self, x, d, blk, key, p, dec, out=None):
        """LN + Linear + GELU + Linear + layer scale + residual in one launch.  A GEMM-pair backward (C = 384 by default) gets its optional
        tensors from the forward's registers: the LayerNorm output as one [M,C] store instead of a LayerNorm pass over d in the backward,
        GELU(hidden) as the second GEMM consumed it."""
        bwd, aux_kind, keep_ln, keep_g = self._saving(p, dec, d.shape[0])
        keep = aux_kind is not None
        outs = K.cnblock_mlp_fwd(d, blk.block[2].weight.data, blk.block[2].bias.data, LN_EPS, self._wc[key + ".mlp"],
                                 blk.block[3].bias.data, blk.block[5].bias.data, self._wc[key + ".gamma"], x,
                                 want_hpre=keep, want_stats=keep, want_xln=keep_ln, want_gact=keep_g, hpre_kind=1 if aux_kind == "dgelu" else 0,
                                 out=out)
        xn, hpre, mean, rstd = outs[:4]
        if dec is None:
            return xn, None
        return xn, BlockSaved(x, d, mean, rstd, hpre, aux_kind, outs[4] if keep_ln else None, outs[-1] if keep_g else None, bwd)

    def _fwd_gemm(self, x, d, blk, key, p, dec, out=None):
        """LayerNorm, then the two pointwise GEMMs with GELU / layer scale + residual in their epilogues; bf16 or (fp8 blocks) e4m3 operands,
        fp32 accumulate.  The 4C-wide side output (the pre-activation, or GELU' of it) is bf16 in both."""
        C, wc, save = p.C, self._wc, dec is not None
        bwd, aux_kind, keep_ln, keep_g = self._saving(p, dec, d.shape[0])
        hpre = torch.empty(x.shape[0], 4 * C, device=x.device, dtype=torch.bfloat16) if save else None
        epi = L.EPI_GELU_DAUX if aux_kind == "dgelu" else L.EPI_GELU
        if p.kind == "fp8":
            ln, mean, rstd = K.layernorm_fwd_fp8(d, blk.block[2].weight.data, blk.block[2].bias.data, LN_EPS, want_stats=save)
            g = L.gemm_nt_fp8(ln, wc[key + ".w1f8"], bias=blk.block[3].bias.data, aux_out=hpre, epi=epi, out_kind=L.OUT_E4M3,
                              alpha_dev=wc[key + ".s1"][1:])
            xn = L.gemm_nt_fp8(g, wc[key + ".w2f8"], out=out, bias=blk.block[5].bias.data, colscale=wc[key + ".gamma"],
                               residual=x, alpha_dev=wc[key + ".s2"][1:])
        else:
            ln, mean, rstd = K.layernorm_fwd(d, blk.block[2].weight.data, blk.block[2].bias.data, LN_EPS, want_stats=save)
            g = L.gemm_nt(ln, wc[key + ".w1"], bias=blk.block[3].bias.data, aux_out=hpre, epi=epi)
            xn = L.gemm_nt(g, wc[key + ".w2"], out=out, bias=blk.block[5].bias.data, colscale=wc[key + ".gamma"], residual=x)
        if not save:
            return xn, None
        return xn, BlockSaved(x, d, mean, rstd, hpre, aux_kind, ln if keep_ln else None, g if keep_g else None, bwd)

    # ---- forward / backward over one micro-batch -----------------------------------------------------------
    def _forward_mb(self, img, plan, dec, sched=None, tabs=None):
        """plan: the tower's BlockPlans as the recorded forward this pass belongs to read them; dec: that forward's SaveDecision, or None
        when this pass saves nothing (no gradient wanted, or a checkpointed micro-batch whose forward runs again in the backward).
        sched: this micro-batch's stochastic-depth Schedule (convnext_sd.schedule) or None.  With one, the features leave in the order
        sched.perm (the caller routes them back), and a block that keeps n_k of the n images runs on the first n_k after the schedule's
        swaps; its record holds views of that prefix.  tabs: this micro-batch's augmentation tables (geom, tone) on the device, or None."""
        f, wc = self.model.features, self._wc
        save = dec is not None
        n, _, H, W = img.shape
        h, w_ = H // 4, W // 4
        saved = {"maps": [(h, w_)]}                 # map size per stage: floored at every stride, so the backward reads them back
        steps = table = None
        if sched is not None:
            steps = sched.steps
            if sched.table:                         # every block's pairs in ONE upload; the host copy is what mmg_image_swap validates
                host = (ctypes.c_int * len(sched.table))(*sched.table)
                table = (torch.tensor(sched.table, dtype=torch.int32, device=img.device), host)
            saved["sd"] = (steps, table)
        b = 0
        p0 = K.patchify(img, 4, self.kp, self.scale16, *(tabs or (None, None)))
        if K.stem_fused_enabled() and K.stem_supported(self.dims[0], self.kp):
            # conv GEMM + LayerNorm in one launch (csrc/stem.hip): s0 = p0 w^T + bias is rounded to bf16 on chip and never stored;
            # the record's None tells the backward to recompute it from p0
            s0 = None
            x, mean, rstd = K.stem_fwd(p0, wc["stem.w"], f[0][0].bias.data, f[0][1].weight.data, f[0][1].bias.data, LN_EPS, want_stats=save)
        else:                                       # three launches (MMG_STEM_FUSED=0, or a width the fused kernels do not have)
            s0 = L.gemm_nt(p0, wc["stem.w"], bias=f[0][0].bias.data)
            x, mean, rstd = K.layernorm_fwd(s0, f[0][1].weight.data, f[0][1].bias.data, LN_EPS, want_stats=save)
        if save:
            saved["stem"] = (p0, s0, mean, rstd)
        for si, p in enumerate(plan):
            mlp = self._fwd_fused if fused_forward(p, save) else self._fwd_gemm
            for bi, blk in enumerate(f[1 + 2 * si]):
                key = f"{si}.{bi}"
                step = steps[b] if steps is not None else None
                b += 1
                if step is None or step.n_k == n:
                    d = K.dwconv7(x, wc[key + ".w49"], blk.block[0].bias.data, n, h, w_, p.C)
                    x, rec = mlp(x, d, blk, key, p, dec)
                elif step.n_k == 0:                 # dropped for every image of this micro-batch: the identity, nothing saved
                    rec = None
                else:
                    # x is the previous layer's fresh output and no record holds it (the stem keeps its own input and statistics, a
                    # downsample layer its input, a block its input - never its output), so the images may change places in it
                    K.image_swap_(x, n, *(table or (None, None)), len(step.pairs), step.offset)
                    n_k, Mk = step.n_k, step.n_k * h * w_
                    xk, out = x[:Mk], torch.empty_like(x)
                    d = K.dwconv7(xk, wc[key + ".w49"], blk.block[0].bias.data, n_k, h, w_, p.C)
                    _, rec = mlp(xk, d, blk, key, p, dec, out=out[:Mk])
                    K.image_copy(x, out, n, n_k, n - n_k)
                    x = out
                if save:
                    saved[key] = rec
            if si < 3:
                lnm = f[2 + 2 * si][0]
                ld, mean, rstd = K.layernorm_fwd(x, lnm.weight.data, lnm.bias.data, LN_EPS, patch_hw=(h, w_), want_stats=save)
                xn = L.gemm_nt(ld, wc[f"ds{si}.w"], bias=f[2 + 2 * si][1].bias.data)
                if save:
                    saved[f"ds{si}"] = (x, mean, rstd, ld)
                x = xn
                h, w_ = h // 2, w_ // 2
                saved["maps"].append((h, w_))
        feat = K.avgpool_fwd(x, n, h * w_, self.dims[-1])
        saved["shape"] = (n, H, W)
        return feat, saved

    # ---- one block's MLP, backward: (dx, rec, blk, key, tmp) -> dd, the gradient w.r.t. the depthwise output -----------------
    def _ln_bwd(self, dln, d, mean, rstd, blk):
        return K.layernorm_bwd(dln, d, mean, rstd, blk.block[2].weight.data, self._g(blk.block[2], "weight"), self._g(blk.block[2], "bias"))

    def _bwd_bwdw(self, dx, rec, blk, key, tmp):
        """Stage 1: data path AND both weight gradients in two launches that read dx, d and write dd - the g / dh tensors ([M,4C] each) of
        the fused form below and its two weight-gradient GEMMs do not exist."""
        packed, b1f = self._wc[key + ".bwdw"]
        return K.cnblock_bwdw(dx, rec.d, blk.block[2].weight.data, blk.block[2].bias.data, LN_EPS, packed, b1f,
                              self._g(blk.block[3], "weight"), self._g(blk.block[3], "bias"), tmp[key + ".dw2raw"], tmp[key + ".db2raw"],
                              self._g(blk.block[2], "weight"), self._g(blk.block[2], "bias"))

    def _bwd_fused(self, dx, rec, blk, key, tmp):
        """Fused data path (hidden row recomputed on chip, or - rec.aux - read back) + the two weight-gradient GEMMs."""
        # C <= 128: the LayerNorm backward rides in the epilogue (`dd` comes back instead of d LN-out); wider blocks have no registers
        # left for it
        fuse_ln = rec.d.shape[1] <= 128
        dh, g, ln, dln, mean, rstd = K.cnblock_mlp_bwd(
            dx, rec.d, blk.block[2].weight.data, blk.block[2].bias.data, LN_EPS, self._wc[key + ".mlpb"], blk.block[3].bias.data, rec.aux,
            ln_grads=(self._g(blk.block[2], "weight"), self._g(blk.block[2], "bias")) if fuse_ln else None)
        L.gemm_tn_acc(dx, g, tmp[key + ".dw2raw"], colsum=tmp[key + ".db2raw"])
        del g
        L.gemm_tn_acc(dh, ln, self._g(blk.block[3], "weight"), colsum=self._g(blk.block[3], "bias"))
        del ln, dh
        return dln if fuse_ln else self._ln_bwd(dln, rec.d, mean, rstd, blk)

    def _bwd_fp8(self, dx, rec, blk, key, tmp):
        """8-bit backward (config C5): rec.aux holds GELU'(h) (bf16), rec.ln / rec.g the e4m3 operands of the forward GEMMs."""
        wc = self._wc
        # (delayed scaling from the second use on: the scale of this block's gradient comes from its previous quantisation - one pass)
        # (+ the bias gradient of the second Linear = column sums of the bf16 gradient itself, in the same pass over it)
        dy8, sdy = K.quantize_e5m2(dx, self._e5m2_state.setdefault(key, {}) if self.fp8_delayed else None, colsum=tmp[key + ".db2raw"])
        dh8 = L.gemm_nt_fp8_bwd(dy8, wc[key + ".w2gt8"], aux_in=rec.aux, epi=L.EPI_MUL_AUX, out_kind=L.OUT_E5M2,
                                alpha_dev=wc[key + ".s2gt"][1:])               # e5m2 at dy's scale: (acc / s_w) * GELU'
        L.gemm_tn_fp8_acc(dy8, rec.g, tmp[key + ".dw2raw"], alpha_dev=sdy[1:])
        L.gemm_tn_fp8_acc(dh8, rec.ln, self._g(blk.block[3], "weight"), alpha_dev=sdy[1:], colsum=self._g(blk.block[3], "bias"))
        dln = L.gemm_nt_fp8_bwd(dh8, wc[key + ".w1t8"], alpha_dev=wc[key + ".s1t"][1:], alpha_dev2=sdy[1:])
        del dh8, dy8
        return self._ln_bwd(dln, rec.d, rec.mean, rec.rstd, blk)

    def _bwd_gemm(self, dx, rec, blk, key, tmp):
        """GEMM pair, bf16, on the saved 4C-wide tensor(s)."""
        wc = self._wc
        if rec.g is not None:                  # the forward kept GELU(h): GELU' only (half the epilogue's arithmetic and stores)
            g = rec.g
            # ... and (aux_kind "dgelu") GELU'(h) in place of h: one multiply per element
            dh = L.gemm_nt(dx, wc[key + ".w2gt"], epi=L.EPI_MUL_AUX if rec.aux_kind == "dgelu" else L.EPI_DGELU_ONLY, aux_in=rec.aux)
        else:
            g = torch.empty_like(rec.aux)      # GELU(h), rebuilt by the same epilogue that applies GELU'
            dh = L.gemm_nt(dx, wc[key + ".w2gt"], epi=L.EPI_DGELU, aux_in=rec.aux, aux_out=g)
        L.gemm_tn_acc(dx, g, tmp[key + ".dw2raw"], colsum=tmp[key + ".db2raw"])
        del g
        ln = rec.ln if rec.ln is not None else \
            K.layernorm_fwd(rec.d, blk.block[2].weight.data, blk.block[2].bias.data, LN_EPS, want_stats=False)[0]
        L.gemm_tn_acc(dh, ln, self._g(blk.block[3], "weight"), colsum=self._g(blk.block[3], "bias"))
        del ln
        w1t, lnm = wc[key + ".w1t"], blk.block[2]
        if lnbwd_fused(dh.shape[0], w1t.shape[0], w1t.shape[1], rec.d.shape[1]):
            # dln = dh W1 never reaches memory: the LayerNorm backward rides in the GEMM's epilogue (csrc/gemm_lnbwd.hip)
            dd = K.gemm_nt_lnbwd(dh, w1t, rec.d, rec.mean, rec.rstd, lnm.weight.data, self._g(lnm, "weight"), self._g(lnm, "bias"))
            del dh
            return dd
        dln = L.gemm_nt(dh, w1t)
        del dh
        return self._ln_bwd(dln, rec.d, rec.mean, rec.rstd, blk)

    def _backward_mb(self, dfeat, saved, tmp, final=False, announce=False):
        """final: last micro-batch of this backward - the GEMM-shaped temporaries of a stage are folded into the torch-layout
        gradients as soon as the stage has passed; announce: it is also the tower's last backward of the step, so the stage's
        gradients are complete and are handed to the gradient all-reduce (ParamArena.mark_ready) while the earlier, larger
        feature maps are still in backward."""
        f, wc, A = self.model.features, self._wc, self._arena
        n, H, W = saved["shape"]
        maps = saved["maps"]
        steps, table = saved.get("sd", (None, None))
        b = sum(self.depths)
        h, w_ = maps[3]
        dx = K.avgpool_bwd(dfeat, n, h * w_, self.dims[-1])
        for si in range(3, -1, -1):
            C = self.dims[si]
            if si < 3:
                x, mean, rstd, ld = saved[f"ds{si}"]
                conv, lnm = f[2 + 2 * si][1], f[2 + 2 * si][0]
                L.gemm_tn_acc(dx, ld, tmp[f"ds{si}.dw"], colsum=self._g(conv, "bias"))
                wt = wc[f"ds{si}.wt"]
                h, w_ = maps[si]                   # (odd sizes: the dropped last row / column gets a zero gradient here)
                if lnbwd_fused(dx.shape[0], wt.shape[0], wt.shape[1], C, (h, w_)):
                    # even maps: dld = dx Wt stays on chip, one launch (odd maps need dx = 0 in pixels no GEMM row visits)
                    dx = K.gemm_nt_lnbwd(dx, wt, x, mean, rstd, lnm.weight.data, self._g(lnm, "weight"), self._g(lnm, "bias"),
                                         patch_hw=(h, w_))
                else:
                    dld = L.gemm_nt(dx, wt)
                    dx = K.layernorm_bwd(dld, x, mean, rstd, lnm.weight.data, self._g(lnm, "weight"), self._g(lnm, "bias"),
                                         patch_hw=(h, w_))
                    del dld
            for bi in range(self.depths[si] - 1, -1, -1):
                blk = f[1 + 2 * si][bi]
                key = f"{si}.{bi}"
                rec = saved[key]
                b -= 1
                step = steps[b] if steps is not None else None
                if step is None or step.n_k == n:
                    dd = getattr(self, "_bwd_" + rec.bwd)(dx, rec, blk, key, tmp)
                    K.dwconv7_wgrad(rec.x, dd, tmp[key + ".dw49"], self._g(blk.block[0], "bias"), n, h, w_, C)
                    dx = K.dwconv7(dd, wc[key + ".w49"], None, n, h, w_, C, add=dx, flip=True)
                    del dd
                elif step.n_k:                      # (n_k = 0: dx passes through, the block's parameters get nothing)
                    # the forward's mirror: the block's backward on the kept prefix, the tail copied through, the swap undone
                    n_k, Mk = step.n_k, step.n_k * h * w_
                    dxk, dxn = dx[:Mk], torch.empty_like(dx)
                    dd = getattr(self, "_bwd_" + rec.bwd)(dxk, rec, blk, key, tmp)
                    K.dwconv7_wgrad(rec.x, dd, tmp[key + ".dw49"], self._g(blk.block[0], "bias"), n_k, h, w_, C)
                    K.dwconv7(dd, wc[key + ".w49"], None, n_k, h, w_, C, add=dxk, flip=True, out=dxn[:Mk])
                    del dd, dxk
                    K.image_copy(dx, dxn, n, n_k, n - n_k)
                    dx = K.image_swap_(dxn, n, *(table or (None, None)), len(step.pairs), step.offset)
            if final:
                self._finalize_stage(tmp, si)
                if announce:
                    A.mark_ready((f"features.{1 + 2 * si}.",) + ((f"features.{2 + 2 * si}.",) if si < 3 else ()))
        p0, s0, mean, rstd = saved["stem"]
        if s0 is None:                      # the forward took the fused launch: LayerNorm backward + both weight gradients in one, nothing [M,C] written
            K.stem_bwd(dx, p0, wc["stem.w"], f[0][0].bias.data, f[0][1].weight.data, mean, rstd, tmp["stem.dw"], self._g(f[0][0], "bias"),
                       self._g(f[0][1], "weight"), self._g(f[0][1], "bias"))
        else:
            ds0 = K.layernorm_bwd(dx, s0, mean, rstd, f[0][1].weight.data, self._g(f[0][1], "weight"), self._g(f[0][1], "bias"))
            L.gemm_tn_acc(ds0, p0, tmp["stem.dw"], colsum=self._g(f[0][0], "bias"))
        if final:                           # fold the GEMM-shaped stem temporary ([C0, kp], zero-padded tail) into the torch-layout gradient
            fold_conv_grad(tmp["stem.dw"], self._g(f[0][0], "weight"), self.dims[0], self.in_chans, 4, 4)

    def _alloc_tmp(self, device):
        z = lambda *s: torch.zeros(*s, device=device, dtype=torch.float32)   # noqa: E731
        tmp = {"stem.dw": z(self.dims[0], self.kp)}
        for si in range(4):
            C = self.dims[si]
            for bi in range(self.depths[si]):
                key = f"{si}.{bi}"
                tmp[key + ".dw2raw"], tmp[key + ".db2raw"], tmp[key + ".dw49"] = z(C, 4 * C), z(C), z(49, C)
            if si < 3:
                tmp[f"ds{si}.dw"] = z(self.dims[si + 1], 4 * C)
        return tmp

    def _finalize_stage(self, tmp, si):
        """Fold stage si's GEMM-shaped temporaries (and those of the downsample layer behind it) into the torch-layout gradients
        (layer scale, conv layouts)."""
        f = self.model.features
        C = self.dims[si]
        scales = self._wc["sd.scales"]
        for bi, blk in enumerate(f[1 + 2 * si]):
            key = f"{si}.{bi}"
            # stochastic depth: the kernels ran on gamma_eff = gamma * s_b.  Given gamma_eff, dW2 and db2 come out right; the third result is
            # d/d(gamma_eff), and d/d(gamma) is s_b times it: through a [C] temporary
            s = scales[sum(self.depths[:si]) + bi] if scales is not None else 1.0
            dgamma = self._g(blk, "layer_scale") if s == 1.0 else torch.zeros(C, device=tmp[key + ".dw2raw"].device, dtype=torch.float32)
            call("mmg_layerscale_finalize", ptr(blk.block[5].weight.data), ptr(blk.block[5].bias.data),
                 ptr(self._wc[key + ".gamma"]), ptr(tmp[key + ".dw2raw"]), ptr(tmp[key + ".db2raw"]),
                 ptr(self._g(blk.block[5], "weight")), ptr(self._g(blk.block[5], "bias")),
                 ptr(dgamma), C, 4 * C, stream())
            if s != 1.0:
                K.scaled_add_(self._g(blk, "layer_scale"), dgamma, s)
            call("mmg_grad_relayout", ptr(tmp[key + ".dw49"]), ptr(self._g(blk.block[0], "weight")), 1, C, 1, 7, 7, C,
                 stream())
        if si < 3:
            fold_conv_grad(tmp[f"ds{si}.dw"], self._g(f[2 + 2 * si][1], "weight"), self.dims[si + 1], C, 2, 2)

    # ---- public -----------------------------------------------------------------------------------------------
    def feature_map_shape(self, H, W):
        """(h, w) of the last stage for an H x W input (floor at every stride, e.g. 1906 x 818 -> 59 x 25)."""
        h, w = H // 4, W // 4
        for _ in range(3):
            h, w = h // 2, w // 2
        return h, w

    def forward(self, images, sample_ids=None):
        """images: [n, Cin, H, W] (any H, W >= 32; fp32 in [0,1], or raw uint16 / uint8, which stay as they are), or a list / tuple of
        [Cin, H_i, W_i] tensors whose sizes may differ: those are grouped by size (`group_by_size`), every group runs in micro-batches of its
        own, and row i of the result belongs to images[i].
        sample_ids (stochastic depth and augmentation): the number under which image i draws, default i - its position in this input."""
        plan = None
        if isinstance(images, (list, tuple)):
            if not images or any(not torch.is_tensor(t) or t.dim() != 3 for t in images):
                raise ValueError("a list of images must hold [Cin, H, W] tensors")
            for t in images:
                _hip.require_gpu(t)
                if t.shape[-2] < 32 or t.shape[-1] < 32:
                    raise ValueError(f"ConvNeXt needs at least 32x32 pixels, got {tuple(t.shape)}")
            plan = group_by_size([tuple(t.shape[-2:]) for t in images], self.micro_batch)
            device = images[0].device
        else:
            _hip.require_gpu(images)
            if images.shape[-2] < 32 or images.shape[-1] < 32:
                raise ValueError(f"ConvNeXt needs at least 32x32 pixels, got {tuple(images.shape)}")
            device = images.device
        anchor = self._record_forward(device)
        seed = None
        if self.stochastic_depth_active():      # one seed per forward; a checkpointed recomputation reuses the schedules made from it
            if self.next_drop_seed is not None:
                seed, self.next_drop_seed = int(self.next_drop_seed), None
            else:
                seed = self._drop_seeds.draw()
            ids = list(range(len(images))) if sample_ids is None else [int(i) for i in sample_ids]
            if len(ids) != len(images):
                raise ValueError(f"sample_ids names {len(ids)} images, the input holds {len(images)}")
            seed = (seed, ids)
        aug = self._draw_augment(len(images), sample_ids)       # one draw per forward; the rows go with the forward's record
        if plan is None:
            return _ConvNextFn.apply(self, as_pixels(images).contiguous(), anchor, None, seed, aug)
        return _ConvNextFn.apply(self, [as_pixels(t) for t in images], anchor, plan, seed, aug)


def group_by_size(sizes, micro_batch):
    """sizes: one (H, W) per image -> (micro_batches, inverse).  Images of one size form a group; groups come in the order in which their size
    first appears, the images inside a group in input order, and every group is cut into micro-batches of at most `micro_batch` images
    (lists of input indices).  Concatenating the micro-batches gives the processing order; inverse[i] is the position of image i in it, so
    `processed[inverse]` is in input order."""
    if micro_batch < 1:
        raise ValueError(f"micro_batch must be positive, got {micro_batch}")
    groups = {}
    for i, hw in enumerate(sizes):
        groups.setdefault(tuple(int(v) for v in hw), []).append(i)          # (dicts keep insertion order: first appearance)
    mbs = [idx[k:k + micro_batch] for idx in groups.values() for k in range(0, len(idx), micro_batch)]
    inverse = [0] * len(sizes)
    for pos, i in enumerate(j for mb in mbs for j in mb):
        inverse[i] = pos
    return mbs, inverse


class _ConvNextFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tower, images, anchor, plan, sd_seed=None, aug=None):
        """sd_seed: None, or (seed, sample ids) of a forward that applies stochastic depth; aug: None, or the (geom rows, tone rows) of a
        forward that augments (Tower._draw_augment)."""
        tower._refresh_working_copies()
        save = anchor is not None
        mb = tower.micro_batch
        ckpt = save and tower.checkpoint
        if plan is None:
            count, device = images.shape[0], images.device
            mbs = [list(range(i, min(i + mb, count))) for i in range(0, count, mb)]
            parts = [(lambda i=i: images[i:i + mb]) for i in range(0, count, mb)]
            alive = [(min(mb, count) if ckpt else count, images.shape[-2], images.shape[-1])]
        else:                               # images of several sizes: one [k, Cin, H, W] tensor per group-micro-batch, built when it is needed
            count, device = len(images), images[0].device
            mbs = plan[0]
            parts = [(lambda idx=idx: K.stack_images([images[j] for j in idx]).contiguous()) for idx in plan[0]]
            by_size = {}
            for idx in plan[0]:
                hw = tuple(images[idx[0]].shape[-2:])
                by_size[hw] = max(by_size.get(hw, 0), len(idx)) if ckpt else by_size.get(hw, 0) + len(idx)
            alive = [(k, hw[0], hw[1]) for hw, k in by_size.items()]
            if ckpt:                        # one micro-batch alive at a time: the largest one decides
                alive = [max(alive, key=lambda a: a[0] * a[1] * a[2])]
        # the plan and the decision on what to keep belong to THIS forward: every pass of it, the recomputation inside its backward included,
        # gets them as arguments (a tower may record several forwards before the first backward)
        maxc = _fused_save_maxc()
        blocks = tower.plan = tuple(p._replace(fused_save_maxc=maxc) for p in tower.plan)
        dec = None
        if save:
            dec = tower._decide_saves(*alive[0], device, ckpt=ckpt and len(parts) > 1, more=alive[1:])
            tower.save_ln, tower.save_gelu, tower.fp8_bwd_now = dec         # (the latest forward's, for whoever reports them: bench.py)
        inverse = plan[1] if plan is not None else list(range(count))
        # augmentation: row i of the tables belongs to input image i; ONE upload in processing order, a slice per micro-batch, carried
        # along with the pixels like the schedules below, so a checkpointed recomputation reads the same rows
        tabs = augment_tables(aug, mbs, device) if aug is not None else [None] * len(mbs)
        if sd_seed is not None:
            # stochastic depth: the mask of a sample is a function of (seed, block, its index in the INPUT); every micro-batch gets its
            # schedule here, once, and carries it along with its pixels (a part is opaque to forward_parts / backward_parts), so the
            # recomputation of a checkpointed part executes the same record
            rates = SD.block_rates(tower.stochastic_depth_prob, tower.depths)
            scheds = [SD.schedule(SD.keep_matrix(sd_seed[0], [sd_seed[1][i] for i in idx], rates)) for idx in mbs]
            parts = [(lambda part=part, sch=sch, tab=tab: (part(), sch, tab)) for part, sch, tab in zip(parts, scheds, tabs)]
            inverse = SD.processing_order(mbs, scheds)[1]
            run = lambda x, saving: tower._forward_mb(x[0], blocks, dec if saving else None, x[1], x[2])      # noqa: E731
        elif aug is not None:
            parts = [(lambda part=part, tab=tab: (part(), None, tab)) for part, tab in zip(parts, tabs)]
            run = lambda x, saving: tower._forward_mb(x[0], blocks, dec if saving else None, None, x[2])      # noqa: E731
        else:
            run = lambda pix, saving: tower._forward_mb(pix, blocks, dec if saving else None)           # noqa: E731
        out, parts = forward_parts(parts, run, ckpt)
        ctx.tower, ctx.parts = tower, parts if save else None
        ctx.plan, ctx.decision = blocks, dec
        ctx.inverse, ctx.sd = None, sd_seed is not None or aug is not None      # (sd: a part is (pixels, schedule, tables))
        if inverse != list(range(count)):
            ctx.inverse = torch.tensor(inverse, device=device)
            out = out.index_select(0, ctx.inverse)             # processing order -> input order
        return out

    @staticmethod
    def backward(ctx, dfeat):
        tower = ctx.tower
        tower._arena.prepare_grads()
        tmp = tower._alloc_tmp(dfeat.device)
        dfeat = dfeat.float().contiguous()
        if ctx.inverse is not None:                                # input order -> processing order
            dfeat = torch.empty_like(dfeat).index_copy_(0, ctx.inverse, dfeat)

        def bwd(d, saved, final):            # final: the GEMM-shaped temporaries are folded, and (the step's last backward) announced
            tower._backward_mb(d, saved, tmp, final=final, announce=final and last_backward(tower))
        again = (lambda x: tower._forward_mb(x[0], ctx.plan, ctx.decision, x[1], x[2])[1]) if ctx.sd else \
            (lambda pix: tower._forward_mb(pix, ctx.plan, ctx.decision)[1])
        backward_parts(ctx.parts, dfeat, again, bwd)
        backward_finished(tower)
        return None, None, None, None, None, None
