"""ViT-B/16 image tower on the HIP kernels (forward + backward), state-dict compatible with torchvision `vit_b_16`.

Not in the reference (its image encoders are ConvNeXt-T / ResNet-50, mmgclip/networks/encoder.py:15,57): BASELINE config C4
asks for it (SURVEY.md §7 decision 2: CLS token + learned absolute positions sized to the configured image, pre-LN
ViT-B/16, 768 features).  Layout follows torchvision.models.VisionTransformer: `conv_proj`, `class_token`,
`encoder.pos_embedding`, `encoder.layers.encoder_layer_{i}.{ln_1, self_attention.{in_proj_weight,in_proj_bias,out_proj},
ln_2, mlp.{0,3}}`, `encoder.ln`; LayerNorm eps 1e-6, erf-GELU, no dropout.  The oracle is oracle/encoders_oracle.vit_forward.

All layers reuse the BERT/ConvNeXt kernels: the 16x16/16 patch convolution is `mmg_patchify` + GEMM, attention is
`mmg_attention_fwd/bwd` without a key mask (whole sequence in LDS) up to S = 256 tokens (224x224 -> 197) and the
flash-style tiled `mmg_attention_long_fwd/bwd` beyond (1024x1024 -> S = 4097, BASELINE config C4).

`patch_dropout` (FLIP / open_clip; mmgclip/patch_dropout.py, csrc/patch_dropout.hip): under train() every image keeps K of its patches and
the class token, drawn once per forward on the device; the kept rows are gathered before the patch-embedding GEMM and every layer runs at
S = 1 + K.  eval() and rate 0 take the code path above unchanged.  `patch_prior="foreground"` makes that draw foreground first
(`mmg_patch_foreground` counts the pixels above `patch_threshold` per patch under the forward's own augmentation geometry,
`mmg_patch_keep_indices_prior` puts the patches with at least `patch_min_pixels` of them in front), and `patch_dropout_eval` keeps the same K
under eval() from the pixels alone.  The default prior, "uniform", launches nothing new.
"""
import torch
import torch.nn as nn

from .. import _hip
from .. import kernels as K
from .. import linalg as L
from .. import patch_dropout as PD
from .._hip import call, ptr, stream
from ..params import backward_finished
from .tower import Tower, as_pixels, augment_tables, backward_parts, conv_weight_rows, fold_conv_grad, forward_parts

LN_EPS = 1e-6


def _tv_layout(image_size, in_chans, hidden, layers, mlp_dim, patch):
    m = nn.Module()
    m.conv_proj = nn.Conv2d(in_chans, hidden, kernel_size=patch, stride=patch)
    m.class_token = nn.Parameter(torch.zeros(1, 1, hidden))
    m.encoder = nn.Module()
    seq = (image_size // patch) ** 2 + 1
    m.encoder.pos_embedding = nn.Parameter(torch.empty(1, seq, hidden).normal_(std=0.02))
    m.encoder.layers = nn.Module()
    for i in range(layers):
        blk = nn.Module()
        blk.ln_1 = nn.LayerNorm(hidden, eps=LN_EPS)
        blk.self_attention = nn.Module()
        blk.self_attention.in_proj_weight = nn.Parameter(torch.empty(3 * hidden, hidden))
        blk.self_attention.in_proj_bias = nn.Parameter(torch.zeros(3 * hidden))
        blk.self_attention.out_proj = nn.Linear(hidden, hidden)
        blk.ln_2 = nn.LayerNorm(hidden, eps=LN_EPS)
        blk.mlp = nn.Sequential(nn.Linear(hidden, mlp_dim), nn.GELU(), nn.Identity(), nn.Linear(mlp_dim, hidden), nn.Identity())
        nn.init.xavier_uniform_(blk.self_attention.in_proj_weight)
        nn.init.xavier_uniform_(blk.mlp[0].weight)
        nn.init.xavier_uniform_(blk.mlp[3].weight)
        nn.init.normal_(blk.mlp[0].bias, std=1e-6)
        nn.init.normal_(blk.mlp[3].bias, std=1e-6)
        setattr(m.encoder.layers, f"encoder_layer_{i}", blk)
    m.encoder.ln = nn.LayerNorm(hidden, eps=LN_EPS)
    fan_in = in_chans * patch * patch
    nn.init.trunc_normal_(m.conv_proj.weight, std=(1.0 / fan_in) ** 0.5)
    nn.init.zeros_(m.conv_proj.bias)
    return m


class ViTTower(Tower):
    """pixels [n, Cin, H, W], fp32 in [0,1] or raw uint16 / uint8 -> class-token features [n, hidden].  augment: as ConvNextTower's."""

    def __init__(self, image_size=224, in_chans=1, hidden=768, layers=12, heads=12, mlp_dim=3072, patch=16, scale16=True,
                 micro_batch=256, checkpoint=False, augment=None, patch_dropout=0.0, patch_prior="uniform", patch_threshold=0.0,
                 patch_min_pixels=1, patch_dropout_eval=False):
        super().__init__()
        self._patch_elements = in_chans * patch * patch     # the most a patch can count (patch_min_pixels' range)
        self.set_augment(augment)
        # FLIP's patch dropout (mmgclip/patch_dropout.py): under train() every image keeps K of its patches and the class token, and every
        # layer runs on 1 + K tokens; eval() sees every patch.  May be reassigned between steps (FLIP's unmasked tuning at the end of a run).
        self.patch_dropout = patch_dropout
        # The foreground prior (mmgclip/patch_dropout.py): the same K, tissue first.  All four may be reassigned between steps, too.
        self._patch_dropout_eval = False
        self.patch_prior, self.patch_threshold, self.patch_min_pixels = patch_prior, patch_threshold, patch_min_pixels
        self.patch_dropout_eval = patch_dropout_eval        # under eval() keep K patches as well, drawn from the pixels alone
        self.last_patch_foreground = None   # (n_foreground int32 [n] on the device, K) of the last forward that drew under the prior
        self.next_patch_drop_seed = None    # tests: force the seed of the next forward that drops patches
        self._patch_drop_seeds = PD.PatchDropSeeds()
        self.checkpoint = checkpoint        # keep only each micro-batch's pixels, re-run its forward inside its backward
        assert hidden == 64 * heads, "the attention kernel is specialised for head_dim 64"
        self.image_size, self.in_chans, self.hidden, self.layers, self.heads = image_size, in_chans, hidden, layers, heads
        self.mlp_dim, self.patch, self.scale16, self.micro_batch = mlp_dim, patch, scale16, micro_batch
        self.seq = (image_size // patch) ** 2 + 1
        self.model = _tv_layout(image_size, in_chans, hidden, layers, mlp_dim, patch)
        self.model_output_dimension = hidden
        self.kp = (patch * patch * in_chans + 31) // 32 * 32

    @property
    def patch_dropout(self):
        return self._patch_dropout

    @patch_dropout.setter
    def patch_dropout(self, rate):
        self._patch_dropout = PD.check_rate(rate)

    @property
    def patch_prior(self):
        return self._patch_prior

    @patch_prior.setter
    def patch_prior(self, prior):
        PD.check_dropout_eval(self._patch_dropout_eval, PD.check_prior(prior))
        self._patch_prior = prior

    @property
    def patch_threshold(self):
        return self._patch_threshold

    @patch_threshold.setter
    def patch_threshold(self, threshold):
        self._patch_threshold = PD.check_threshold(threshold)

    @property
    def patch_min_pixels(self):
        return self._patch_min_pixels

    @patch_min_pixels.setter
    def patch_min_pixels(self, min_pixels):
        self._patch_min_pixels = PD.check_min_pixels(min_pixels, self._patch_elements)

    @property
    def patch_dropout_eval(self):
        return self._patch_dropout_eval

    @patch_dropout_eval.setter
    def patch_dropout_eval(self, flag):
        self._patch_dropout_eval = PD.check_dropout_eval(flag, self._patch_prior)

    def patch_dropout_active(self):
        return self._patch_dropout > 0.0 and (self.training or self._patch_dropout_eval)

    def _draw_patch_drop(self, count, sample_ids, device):
        """One draw per forward: -> (keep int32 [count, K], slot int32 [count, P]) on `device`, made in one launch for the whole input, or None
        when no patch is dropped (eval(), or rate 0: no seed is drawn and nothing is launched).  sample_ids: as Tower._draw_augment's."""
        if not self.patch_dropout_active():
            return None
        seed, ids, P, Kk, keep, slot = self._patch_drop_arguments(count, sample_ids, device)
        call("mmg_patch_keep_indices", seed & 0xFFFFFFFFFFFFFFFF, ptr(ids), count, P, Kk, ptr(keep), ptr(slot), stream())
        return keep, slot

    def _patch_drop_arguments(self, count, sample_ids, device, seed=None):
        """What both draws take: the forward's seed (`seed` if given; else the forced one, else the next of the tower's stream), the sample
        ids on the device (or None), P, K and the empty tables."""
        if seed is not None:
            pass
        elif self.next_patch_drop_seed is not None:
            seed, self.next_patch_drop_seed = int(self.next_patch_drop_seed), None
        else:
            seed = self._patch_drop_seeds.draw()
        P = self.seq - 1
        Kk = PD.keep_count(P, self._patch_dropout)
        if P > PD.MAX_PATCHES:
            raise ValueError(f"patch_dropout draws an image's {P} patches in one workgroup, which holds {PD.MAX_PATCHES}")
        ids = None
        if sample_ids is not None:
            ids = [int(i) for i in sample_ids]
            if len(ids) != count:
                raise ValueError(f"sample_ids names {len(ids)} images, the input holds {count}")
            ids = torch.tensor(ids, dtype=torch.int64).to(device)
        keep = torch.empty(count, Kk, device=device, dtype=torch.int32)
        slot = torch.empty(count, P, device=device, dtype=torch.int32)
        return seed, ids, P, Kk, keep, slot

    def _draw_patch_drop_prior(self, pixels, sample_ids, aug):
        """The foreground-first draw, once per forward for the whole input: -> (keep, slot) as _draw_patch_drop's, and
        self.last_patch_foreground = (n_foreground int32 [n] on the device, K).  pixels: the input as the stem will read it ([n, Cin, H, W],
        contiguous); aug: Tower._draw_augment's rows of this forward or None - the counts are taken under the geometry rows patchify will use
        for the same image.  A row is a pure function of (seed, sample id, the image's pixels, its geometry row): the same under any
        micro_batch, and the tables stay with their part for a checkpointed recomputation.
        Under eval() (patch_dropout_eval) every image draws under seed 0 and sample id 0 with no geometry, and the training stream is not
        touched: the kept set, and so the embedding, is a function of the image's pixels alone."""
        n, Cin, Hh, Ww = pixels.shape
        device = pixels.device
        if self.training:
            seed, ids, P, Kk, keep, slot = self._patch_drop_arguments(n, sample_ids, device)
            geom = torch.tensor(aug[0], dtype=torch.int32).reshape(-1, 4).to(device) if aug is not None else None
        else:
            seed, ids, P, Kk, keep, slot = self._patch_drop_arguments(n, [0] * n, device, seed=0)
            geom = None
        counts = torch.empty(n, P, device=device, dtype=torch.int32)
        nfg = torch.empty(n, device=device, dtype=torch.int32)
        call("mmg_patch_foreground", ptr(pixels), K.PIXEL_KINDS[pixels.dtype], n, Cin, Hh, Ww, self.patch, ptr(geom), self._patch_threshold,
             ptr(counts), stream())
        call("mmg_patch_keep_indices_prior", seed & 0xFFFFFFFFFFFFFFFF, ptr(ids), ptr(counts), self._patch_min_pixels, n, P, Kk, ptr(keep),
             ptr(slot), ptr(nfg), stream())
        self.last_patch_foreground = (nfg, Kk)
        return keep, slot

    def _blk(self, i):
        return getattr(self.model.encoder.layers, f"encoder_layer_{i}")

    def _build_working_copies(self):
        wc = {"conv": K.cast_bf16(conv_weight_rows(self.model.conv_proj.weight.data))}       # [hidden, kp]
        wc["cls"] = K.cast_bf16(self.model.class_token.data.reshape(-1))
        wc["pos"] = K.cast_bf16(self.model.encoder.pos_embedding.data.reshape(self.seq, self.hidden))
        for i in range(self.layers):
            b = self._blk(i)
            for tag, wt in (("qkv", b.self_attention.in_proj_weight.data), ("o", b.self_attention.out_proj.weight.data),
                            ("f1", b.mlp[0].weight.data), ("f2", b.mlp[3].weight.data)):
                wc[f"{i}.{tag}"] = K.cast_bf16(wt)
                wc[f"{i}.{tag}t"] = K.transpose_cast_bf16(wt)
        return wc

    def _forward_mb(self, img, save, tabs=None, drop=None):
        """drop: None, or this micro-batch's (keep [B, K], slot [B, P]) rows of _draw_patch_drop: the kept rows of the patchified pixels are
        gathered BEFORE the patch-embedding GEMM, and every layer runs at S = 1 + K."""
        wc, H, heads = self._wc, self.hidden, self.heads
        B, P = img.shape[0], self.seq - 1
        p0 = K.patchify(img, self.patch, self.kp, self.scale16, *(tabs or (None, None)))
        if drop is not None:
            keep, Kk = drop[0], drop[0].shape[1]
            kept = torch.empty(B * Kk, self.kp, device=img.device, dtype=torch.bfloat16)
            call("mmg_gather_patch_rows", ptr(p0), self.kp, ptr(keep), ptr(kept), B, P, Kk, self.kp, stream())
            p0 = kept
        S = self.seq if drop is None else 1 + Kk
        tok = L.gemm_nt(p0, wc["conv"], bias=self.model.conv_proj.bias.data)
        x = torch.empty(B * S, H, device=img.device, dtype=torch.bfloat16)
        if drop is None:
            call("mmg_vit_assemble_fwd", ptr(tok), ptr(wc["cls"]), ptr(wc["pos"]), ptr(x), B, S, H, stream())
        else:
            call("mmg_vit_assemble_keep_fwd", ptr(tok), ptr(wc["cls"]), ptr(wc["pos"]), ptr(keep), ptr(x), B, P, Kk, H, stream())
        saved = {"p0": p0, "layers": [], "B": B, "S": S, "drop": drop} if save else None
        del tok
        for i in range(self.layers):
            b = self._blk(i)
            y, m1, r1 = K.layernorm_fwd(x, b.ln_1.weight.data, b.ln_1.bias.data, LN_EPS, want_stats=save)
            qkv = L.gemm_nt(y, wc[f"{i}.qkv"], bias=b.self_attention.in_proj_bias.data)
            ctx, lse = K.attention_fwd(qkv, None, B, S, heads, want_lse=save)
            x1 = L.gemm_nt(ctx, wc[f"{i}.o"], bias=b.self_attention.out_proj.bias.data, residual=x)
            z, m2, r2 = K.layernorm_fwd(x1, b.ln_2.weight.data, b.ln_2.bias.data, LN_EPS, want_stats=save)
            hpre = torch.empty(B * S, self.mlp_dim, device=img.device, dtype=torch.bfloat16) if save else None
            g = L.gemm_nt(z, wc[f"{i}.f1"], bias=b.mlp[0].bias.data, epi=L.EPI_GELU, aux_out=hpre)
            x2 = L.gemm_nt(g, wc[f"{i}.f2"], bias=b.mlp[3].bias.data, residual=x1)
            if save:
                saved["layers"].append((x, m1, r1, qkv, ctx, lse, x1, m2, r2, hpre))
            del y, g, z
            x = x2
        ln = self.model.encoder.ln
        out, mf, rf = K.layernorm_fwd(x, ln.weight.data, ln.bias.data, LN_EPS, want_stats=save)
        idx = torch.zeros(B, device=img.device, dtype=torch.int32)
        feat = torch.empty(B, H, device=img.device, dtype=torch.float32)
        call("mmg_gather_rows_fwd", ptr(out), ptr(idx), ptr(feat), B, S, H, stream())
        if save:
            saved["final"] = (x, mf, rf, idx)
        return feat, saved

    def _backward_mb(self, dfeat, saved):
        wc, A, H, heads = self._wc, self._arena, self.hidden, self.heads
        B, S, drop = saved["B"], saved["S"], saved["drop"]
        x, mf, rf, idx = saved["final"]
        ln = self.model.encoder.ln
        dout = K.eos_pool_bwd(dfeat, idx, B, S)
        dx = K.layernorm_bwd(dout, x, mf, rf, ln.weight.data, A.g("encoder.ln.weight"), A.g("encoder.ln.bias"))
        del dout
        for i in range(self.layers - 1, -1, -1):
            b = self._blk(i)
            p = f"encoder.layers.encoder_layer_{i}."
            x, m1, r1, qkv, ctx, lse, x1, m2, r2, hpre = saved["layers"][i]
            # MLP branch: x2 = x1 + W2 gelu(W1 LN2(x1) + b1) + b2
            g = torch.empty_like(hpre)
            dh = L.gemm_nt(dx, wc[f"{i}.f2t"], epi=L.EPI_DGELU, aux_in=hpre, aux_out=g)
            L.gemm_tn_acc(dx, g, A.g(p + "mlp.3.weight"), colsum=A.g(p + "mlp.3.bias"))
            del g
            z, _, _ = K.layernorm_fwd(x1, b.ln_2.weight.data, b.ln_2.bias.data, LN_EPS, want_stats=False)
            L.gemm_tn_acc(dh, z, A.g(p + "mlp.0.weight"), colsum=A.g(p + "mlp.0.bias"))
            del z
            dz = L.gemm_nt(dh, wc[f"{i}.f1t"])
            del dh
            dx1 = K.layernorm_bwd(dz, x1, m2, r2, b.ln_2.weight.data, A.g(p + "ln_2.weight"), A.g(p + "ln_2.bias"),
                                  add=dx)                          # + residual path, fused in the LN-backward kernel
            del dz
            # attention branch: x1 = x + Wo attn(Wqkv LN1(x) + b) + bo
            L.gemm_tn_acc(dx1, ctx, A.g(p + "self_attention.out_proj.weight"), colsum=A.g(p + "self_attention.out_proj.bias"))
            dctx = L.gemm_nt(dx1, wc[f"{i}.ot"])
            dqkv = K.attention_bwd(qkv, None, ctx, lse, dctx, B, S, heads)
            del dctx
            y, _, _ = K.layernorm_fwd(x, b.ln_1.weight.data, b.ln_1.bias.data, LN_EPS, want_stats=False)
            L.gemm_tn_acc(dqkv, y, A.g(p + "self_attention.in_proj_weight"), colsum=A.g(p + "self_attention.in_proj_bias"))
            del y
            dy = L.gemm_nt(dqkv, wc[f"{i}.qkvt"])
            del dqkv
            dx = K.layernorm_bwd(dy, x, m1, r1, b.ln_1.weight.data, A.g(p + "ln_1.weight"), A.g(p + "ln_1.bias"), add=dx1)
            del dy, dx1
            saved["layers"][i] = None
        dtok = torch.empty(B * (S - 1), H, device=dx.device, dtype=torch.bfloat16)
        if drop is None:
            call("mmg_vit_assemble_bwd", ptr(dx), ptr(dtok), ptr(A.g("encoder.pos_embedding")), ptr(A.g("class_token")), B, S, H, stream())
        else:
            call("mmg_vit_assemble_keep_bwd", ptr(dx), ptr(drop[1]), ptr(dtok), ptr(A.g("encoder.pos_embedding")), ptr(A.g("class_token")),
                 B, self.seq - 1, S - 1, H, stream())
        tmp = torch.zeros(H, self.kp, device=dx.device, dtype=torch.float32)
        L.gemm_tn_acc(dtok, saved["p0"], tmp, colsum=A.g("conv_proj.bias"))
        fold_conv_grad(tmp, A.g("conv_proj.weight"), H, self.in_chans, self.patch, self.patch)

    def forward(self, images, sample_ids=None):
        """images: [n, Cin, S, S] (fp32 in [0,1], or raw uint16 / uint8), or a list of [Cin, S, S] images, S = image_size.
        sample_ids (augmentation, patch dropout): the number under which image i draws, default i - its position in this input."""
        if isinstance(images, (list, tuple)):
            if not images or any(not torch.is_tensor(t) or t.dim() != 3 for t in images):
                raise ValueError("a list of images must hold [Cin, H, W] tensors")
            if len({tuple(t.shape) for t in images}) != 1:
                raise ValueError(f"ViT was built for {self.image_size}x{self.image_size} inputs (learned positions): every image of a list must "
                                 f"have that size, got {sorted({tuple(t.shape[-2:]) for t in images})}")
            images = K.stack_images([as_pixels(t) for t in images])
        _hip.require_gpu(images)
        if images.shape[-1] != self.image_size or images.shape[-2] != self.image_size:
            raise ValueError(f"ViT was built for {self.image_size}x{self.image_size} inputs (learned positions), got {tuple(images.shape)}")
        anchor = self._record_forward(images.device)
        pixels = as_pixels(images).contiguous()
        aug = self._draw_augment(images.shape[0], sample_ids)
        self.last_patch_foreground = None
        if self._patch_prior == "foreground" and self.patch_dropout_active():
            drop = self._draw_patch_drop_prior(pixels, sample_ids, aug)
        else:
            drop = self._draw_patch_drop(images.shape[0], sample_ids, images.device)
        return _ViTFn.apply(self, pixels, anchor, aug, drop)


class _ViTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tower, images, anchor, aug=None, drop=None):
        """aug: None, or the (geom rows, tone rows) of a forward that augments (Tower._draw_augment): uploaded once, a slice per micro-batch,
        kept with the part so that a checkpointed recomputation reads the same rows.  drop: None, or the (keep, slot) tables of a forward
        that drops patches (ViTTower._draw_patch_drop): made once on the device, sliced and kept with the part the same way."""
        tower._refresh_working_copies()
        save = anchor is not None
        mb, count = tower.micro_batch, images.shape[0]
        starts = range(0, count, mb)
        tabs = augment_tables(aug, [list(range(i, min(i + mb, count))) for i in starts], images.device) if aug is not None else [None] * len(starts)
        drops = [(drop[0][i:i + mb], drop[1][i:i + mb]) if drop is not None else None for i in starts]
        parts = [(lambda i=i, tab=tab, dr=dr: (images[i:i + mb], tab, dr)) for i, tab, dr in zip(starts, tabs, drops)]
        out, parts = forward_parts(parts, lambda x, saving: tower._forward_mb(x[0], save and saving, x[1], x[2]), save and tower.checkpoint)
        ctx.tower, ctx.parts = tower, parts if save else None
        return out

    @staticmethod
    def backward(ctx, dfeat):
        tower = ctx.tower
        tower._arena.prepare_grads()
        dfeat = dfeat.float().contiguous()
        backward_parts(ctx.parts, dfeat, lambda x: tower._forward_mb(x[0], True, x[1], x[2])[1], lambda d, saved, last: tower._backward_mb(d, saved))
        backward_finished(tower)
        return None, None, None, None, None
