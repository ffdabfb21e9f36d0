"""Training the ConvNeXt tower at native image sizes: any H, W >= 32, odd maps floored at every stride as torch's convolutions floor them,
and batches whose images differ in size.

Tolerances are the project's own, set on square maps (tests/test_towers_gpu.py, tests/test_kernels_gpu.py, tests/test_fullsize_gpu.py); what
the ragged cases measure is written by tests.conftest.measured (committed copy: profiles/r05_measured_tolerances.jsonl)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import encoders_oracle as E
from tests.conftest import measured

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CFG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmg-clip_amd", "configs")
DEPTHS = {"tiny": (3, 3, 9, 3), "base": (3, 3, 27, 3)}


def _r(shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def _close(a, b, rtol, atol):
    np.testing.assert_allclose(a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy(), rtol=rtol, atol=atol)


def _rel(a, b):
    a, b = a.detach().float().cpu().double().flatten(), b.detach().float().cpu().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30)), float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))


def _randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if n.endswith("layer_scale"):
                p.copy_(0.3 + 0.7 * torch.rand(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "LayerNorm.weight" in n or (p.dim() == 1 and n.endswith("weight")):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() >= 2 and "embeddings" not in n:
                p.mul_(2.5)


def _maps(H, W):
    out = [(H // 4, W // 4)]
    for _ in range(3):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


# ---- 1. kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("n,H,W,C", [(2, 9, 12, 96), (3, 6, 11, 192), (1, 5, 7, 384), (2, 7, 5, 64), (2, 119, 102, 96), (2, 59, 25, 192)])
def test_layernorm_backward_through_the_ragged_patchified_layout(dev, n, H, W, C, with_add):
    """mmg_layernorm_bwd with patch != 0 and odd H and / or W: dy is [n (H/2) (W/2), 4C] exactly (its own allocation), the pixels of the dropped
    last row / column get dx = 0 (add's row with `add`) and stay out of dgamma / dbeta.  Reference: fp32 autograd of layer_norm -> crop to even ->
    2x2 unfold.  C = 64: the generic kernel (as does every case with `add`); 96 / 192 / 384: the 24 G kernels; 119 x 102: many workgroups."""
    from mmgclip import kernels as K
    M, h2, w2 = n * H * W, H // 2, W // 2
    x = _r((M, C), dev, 5, 2.0).to(BF)
    gamma, beta = _r((C,), dev, 6).abs() + 0.5, _r((C,), dev, 7)
    y, mean, rstd = K.layernorm_fwd(x, gamma, beta, 1e-6, patch_hw=(H, W))
    assert y.shape == (n * h2 * w2, 4 * C)
    dyp = _r((n * h2 * w2, 4 * C), dev, 8).to(BF).clone()
    add = _r((M, C), dev, 9).to(BF) if with_add else None
    start = _r((2, C), dev, 10)                                   # dgamma / dbeta accumulate: start from a non-zero buffer
    dg, db = start[0].clone(), start[1].clone()
    dx = K.layernorm_bwd(dyp, x, mean, rstd, gamma, dg, db, patch_hw=(H, W), add=add)
    xr = x.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (C,), gr, br, 1e-6).reshape(n, H, W, C)[:, :2 * h2, :2 * w2]
    ref = ref.reshape(n, h2, 2, w2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(n * h2 * w2, 4 * C)
    _close(y, ref, 1e-2, 2e-2)
    ref.backward(dyp.float())
    want = xr.grad + (add.float() if with_add else 0.0)
    _close(dx, want, 2e-2, 2e-2)
    dropped = torch.zeros(n, H, W, dtype=torch.bool, device=dev)
    dropped[:, 2 * h2:], dropped[:, :, 2 * w2:] = True, True
    dropped = dropped.reshape(M)
    assert int(dropped.sum()) == n * (H * W - 4 * h2 * w2) and int(dropped.sum()) > 0
    if with_add:
        assert torch.equal(dx[dropped], add[dropped])
    else:
        assert (dx[dropped] == 0).all()
    assert (dx[~dropped].float().abs().sum(-1) > 0).all()         # every live row written
    live = M - int(dropped.sum())
    _close(dg - start[0], gr.grad, 1e-3, 1e-2 * live ** 0.5 * 0.05 + 1e-3)
    _close(db - start[1], br.grad, 1e-3, 1e-3 * live ** 0.5)


# ---- 2. tower against the oracle ------------------------------------------------------------------------------------------------------
def _tower_vs_oracle(dev, variant, n, H, W, fp8=False, images=None, micro_batch=2):
    """Features and every parameter gradient of `(feat * wgt).sum()` on the device and on the fp32 CPU oracle (same weights, same pixels)."""
    from mmgclip.networks.encoder import ConvNextBaseEncoder, ConvNextTinyEncoder
    torch.manual_seed(0)
    tower = (ConvNextTinyEncoder if variant == "tiny" else ConvNextBaseEncoder)(micro_batch=micro_batch, fp8=fp8)
    _randomize(tower, 1)
    sd = {k[len("model."):]: v.clone() for k, v in tower.state_dict().items()}
    img = torch.rand(n, 1, H, W, generator=torch.Generator().manual_seed(2))
    wgt = torch.randn(n, tower.model_output_dimension, generator=torch.Generator().manual_seed(3))
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    kw = dict(fp8_min_channels=tower.fp8_min_channels, fp8_backward=True) if fp8 else {}
    pooled, _ = E.convnext_forward(osd, img, depths=DEPTHS[variant], **kw)
    (pooled.flatten(1) * wgt).sum().backward()
    tower = tower.to(dev)
    feat = tower(img.to(dev))
    fr, fc = _rel(feat, pooled.flatten(1))
    (feat * wgt.to(dev)).sum().backward()
    worst = {name: _rel(p.grad, osd[name].grad) for name, p in tower.model.named_parameters()}
    return tower, fr, fc, worst


BF16_CASES = [("tiny", 3, 77, 50),       # maps 19x12, 9x6, 4x3, 2x1: a row or column is dropped at three levels
              ("tiny", 2, 100, 70),      # 25x17: both odd at stage 1
              ("tiny", 2, 238, 102),     # 1906 x 818 at 1/8: 59x25, 29x12, 14x6, 7x3
              ("tiny", 1, 238, 258),     # 59x64: M % 64 == 0, the stage-1 backward runs on cnblock_bwdw on a ragged image
              ("tiny", 2, 476, 408),     # 119x102 >= 96^2: the matrix-core depthwise kernel in both directions on a map that is no multiple of 16
              ("base", 2, 77, 50)]


@pytest.mark.parametrize("variant,n,H,W", BF16_CASES)
def test_convnext_tower_forward_backward_at_ragged_sizes(dev, variant, n, H, W):
    """tests/test_towers_gpu.py::test_convnext_tower_forward_backward at sizes that are no multiples of 32, at its bars (features rel < 1.5e-2,
    cosine > 0.9999; every gradient cosine > 0.999, rel < 4e-2)."""
    from mmgclip import kernels as K
    h1, w1 = _maps(H, W)[0]
    if (H, W) == (238, 258):
        assert K.cnblock_bwdw_supported(96, n * h1 * w1)
    if (H, W) == (100, 70):
        assert not K.cnblock_bwdw_supported(96, n * h1 * w1) and not K.cnblock_bwdw_supported(96, h1 * w1)
    if (H, W) == (476, 408):
        assert (h1, w1) == (119, 102) and K.dwconv_mfma_pays(n, h1, w1, 96, False) and K.dwconv_mfma_pays(n, h1, w1, 96, True)
    tower, fr, fc, worst = _tower_vs_oracle(dev, variant, n, H, W)
    assert tower.feature_map_shape(H, W) == _maps(H, W)[3]
    gr, gc = max(v[0] for v in worst.values()), min(v[1] for v in worst.values())
    print("native size", variant, n, H, W, "feat rel", fr, "cos", fc, "grad rel max", gr, "cos min", gc)
    measured("convnext_native_size", variant=variant, H=H, W=W, n=n, feat_rel=fr, feat_cos=fc, grad_rel_max=gr, grad_cos_min=gc)
    assert fr < 1.5e-2 and fc > 0.9999, (fr, fc)
    bad = {k: v for k, v in worst.items() if not (v[1] > 0.999 and v[0] < 4e-2)}
    assert not bad, f"{len(bad)} of {len(worst)} gradients off: {list(bad.items())[:8]}"


def test_convnext_base_fp8_forward_backward_at_a_ragged_size(dev):
    """ConvNeXt-B with 8-bit GEMMs in both directions (blocks with C >= 256) at 100 x 70 against the oracle that rounds the same tensors, at the
    bars of test_convnext_fp8_forward_matches_the_fp8_oracle (features rel < 0.1, cosine > 0.995) and
    test_convnext_fp8_backward_matches_the_fp8_oracle (every gradient cosine > 0.94, rel < 0.35) for towers with e4m3 beyond the last stage."""
    tower, fr, fc, worst = _tower_vs_oracle(dev, "base", 2, 100, 70, fp8=True)
    assert tower.fp8_bwd and tower.fp8_bwd_now and tower.fp8_min_channels < tower.dims[-1]
    assert sum(d for d, p in zip(tower.depths, tower.plan) if p.fp8_bwd_weights) == sum(d for d, c in zip(tower.depths, tower.dims) if c >= tower.fp8_min_channels)
    gr, gc = max(v[0] for v in worst.values()), min(v[1] for v in worst.values())
    print("native size fp8 base 100x70 feat rel", fr, "cos", fc, "grad rel max", gr, "cos min", gc)
    measured("convnext_native_size", variant="base_fp8", H=100, W=70, n=2, feat_rel=fr, feat_cos=fc, grad_rel_max=gr, grad_cos_min=gc)
    assert fr < 0.1 and fc > 0.995, (fr, fc)
    bad = {k: v for k, v in worst.items() if not (v[1] > 0.94 and v[0] < 0.35)}
    assert not bad, f"{len(bad)} gradients off: {list(bad.items())[:8]}"


# ---- 3. equalities --------------------------------------------------------------------------------------------------------------------
def _run(tower, img, wgt):
    feat = tower(img)
    (feat * wgt).sum().backward()
    return feat.detach().clone(), {n: p.grad.detach().clone() for n, p in tower.model.named_parameters()}


def test_ragged_size_micro_batch_independence(dev):
    """n = 4 at 100 x 70: one micro-batch of 4 == two of 2 == 3 + 1 (a ragged last micro-batch).  A micro-batch's images never mix in the forward:
    features bit-identical; gradients as in test_convnext_256_images_in_one_micro_batch_equals_four_of_64 (rel < 2e-3: order of fp32 atomics)."""
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    torch.manual_seed(0)
    img = torch.rand(4, 1, 100, 70, generator=torch.Generator().manual_seed(1)).to(dev)
    wgt = torch.randn(4, 768, generator=torch.Generator().manual_seed(2)).to(dev)
    state, res = None, {}
    for mb in (4, 2, 3):
        tower = ConvNextTinyEncoder(micro_batch=mb)
        if state is None:
            state = {k: v.clone() for k, v in tower.state_dict().items()}
        tower.load_state_dict(state)
        res[mb] = _run(tower.to(dev), img, wgt)
    assert torch.isfinite(res[4][0]).all()
    for mb in (2, 3):
        assert torch.equal(res[mb][0], res[4][0]), mb
        for n, g in res[mb][1].items():
            assert _rel(g, res[4][1][n])[0] < 2e-3, (mb, n)


def test_ragged_size_gradient_checkpointing_equals_plain_backward(dev, monkeypatch):
    """test_convnext_gradient_checkpointing_equals_plain_backward at n = 4, 100 x 70 (default initialisation, micro-batches of 2, every micro-batch
    recomputed / the last one kept): features rel < 1e-5, every gradient rel < 2e-3; the checkpointed forward holds the pixels only
    (< 0.25 of the plain forward's activations; with the last of the TWO micro-batches kept, less than the plain forward's)."""
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    torch.manual_seed(0)
    img = torch.rand(4, 1, 100, 70, generator=torch.Generator().manual_seed(1)).to(dev)
    wgt = torch.randn(4, 768, generator=torch.Generator().manual_seed(2)).to(dev)
    ref = ConvNextTinyEncoder(micro_batch=2)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    out = {}
    for ck in (False, "0", "1"):
        monkeypatch.setenv("MMG_CKPT_KEEP_LAST", ck or "1")
        tower = ConvNextTinyEncoder(micro_batch=2, checkpoint=bool(ck))
        tower.load_state_dict(state)
        tower = tower.to(dev)
        tower(img[:2]).sum().backward()                   # materialise arenas / working copies before measuring
        tower.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        feat = tower(img)
        held = torch.cuda.memory_allocated() - base
        (feat * wgt).sum().backward()
        torch.cuda.synchronize()
        out[ck] = (feat.detach().clone(), {n: p.grad.detach().clone() for n, p in tower.model.named_parameters()}, held)
        del tower, feat
    for ck in ("0", "1"):
        assert _rel(out[ck][0], out[False][0])[0] < 1e-5
        for n, g in out[ck][1].items():
            assert _rel(g, out[False][1][n])[0] < 2e-3, (ck, n)
    assert out["0"][2] < 0.25 * out[False][2], (out["0"][2], out[False][2])
    assert out["1"][2] < out[False][2], (out["1"][2], out[False][2])


# ---- 4. mixed sizes -------------------------------------------------------------------------------------------------------------------
MIXED = [(100, 70), (77, 50), (100, 70), (64, 64), (77, 50)]


def test_batch_of_images_of_different_sizes(dev):
    """A list of 5 images of three sizes, micro_batch = 2: feature row i == (bit for bit) the feature of image i when its size group runs alone as
    a 4-D tensor; parameter gradients == the sum of the per-group runs' (rel < 2e-3: order of fp32 atomics) and match the oracle (one
    convnext_forward per group, gradients summed) at the square-map bars."""
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    from mmgclip.networks.convnext import group_by_size
    torch.manual_seed(0)
    tower = ConvNextTinyEncoder(micro_batch=2)
    _randomize(tower, 1)
    sd = {k[len("model."):]: v.clone() for k, v in tower.state_dict().items()}
    g = torch.Generator().manual_seed(2)
    imgs = [torch.rand(1, H, W, generator=g) for H, W in MIXED]
    wgt = torch.randn(len(MIXED), 768, generator=torch.Generator().manual_seed(3))
    groups = {}
    for i, hw in enumerate(MIXED):
        groups.setdefault(hw, []).append(i)
    assert group_by_size(MIXED, 2)[0] == [[0, 2], [1, 4], [3]]
    # oracle: one forward per group, gradients summed
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ofeat = torch.zeros(len(MIXED), 768)
    for hw, idx in groups.items():
        pooled, _ = E.convnext_forward(osd, torch.stack([imgs[i] for i in idx]), depths=DEPTHS["tiny"])
        (pooled.flatten(1) * wgt[idx]).sum().backward()
        ofeat[idx] = pooled.flatten(1).detach()
    tower = tower.to(dev)
    feat, grads = _run(tower, [t.to(dev) for t in imgs], wgt.to(dev))
    assert feat.shape == (len(MIXED), 768)
    # every group alone, as a 4-D tensor
    tower.zero_grad(set_to_none=True)
    for hw, idx in groups.items():
        f = tower(torch.stack([imgs[i] for i in idx]).to(dev))
        (f * wgt[idx].to(dev)).sum().backward()                       # (gradients accumulate over the groups)
        assert torch.equal(f.detach(), feat[idx]), hw
    for n, p in tower.model.named_parameters():
        assert _rel(grads[n], p.grad)[0] < 2e-3, n
    fr, fc = _rel(feat, ofeat)
    worst = {n: _rel(grads[n], osd[n].grad) for n in grads}
    gr, gc = max(v[0] for v in worst.values()), min(v[1] for v in worst.values())
    print("native size mixed feat rel", fr, "cos", fc, "grad rel max", gr, "cos min", gc)
    measured("convnext_native_size", variant="tiny_mixed", H=0, W=0, n=len(MIXED), feat_rel=fr, feat_cos=fc, grad_rel_max=gr, grad_cos_min=gc)
    assert fr < 1.5e-2 and fc > 0.9999, (fr, fc)
    bad = {k: v for k, v in worst.items() if not (v[1] > 0.999 and v[0] < 4e-2)}
    assert not bad, f"{len(bad)} of {len(worst)} gradients off: {list(bad.items())[:8]}"
    # a 4-D tensor and the same images as a list: the same bits
    with torch.no_grad():
        same = torch.rand(3, 1, 100, 70, generator=g).to(dev)
        assert torch.equal(tower(same), tower(list(same)))
    # checkpointing re-stacks a group-micro-batch's pixels in the backward: same gradients
    tower.zero_grad(set_to_none=True)
    tower.checkpoint = True
    feat_c, grads_c = _run(tower, [t.to(dev) for t in imgs], wgt.to(dev))
    assert _rel(feat_c, feat)[0] < 1e-5
    for n in grads:
        assert _rel(grads_c[n], grads[n])[0] < 2e-3, n


# ---- 5. whole model -------------------------------------------------------------------------------------------------------------------
def test_whole_model_trains_at_a_rectangular_native_size_and_on_mixed_sizes(dev, tmp_path, monkeypatch):
    """MMGCLIP from the ConvNeXt-T pixel config with image_size [100, 70] (small BERT, default initialisation): one ClassifierExperiment.train epoch
    on the synthetic loader built as train.py builds it - the first loss is finite and within 0.5 of ln(batch) (the bar of
    test_c4_c5_whole_step_at_per_gpu_batch), every trainable parameter has a finite gradient and (the unused BERT pooler apart) moved.  Then the same with batch["image"] as a
    list of images of two sizes."""
    import train
    from mmgclip.config import compose
    from mmgclip.dataset.synthetic import SyntheticLoader, synthetic_batch
    from mmgclip.experiments.experiments_controller import create_experiment
    from mmgclip.networks import bert
    orig = bert.BertConfigLite.__init__

    def small(self, **kw):
        kw.setdefault("num_hidden_layers", 2)
        kw.setdefault("vocab_size", 3000)
        orig(self, **kw)
    monkeypatch.setattr(bert.BertConfigLite, "__init__", small)
    batch = 8
    cfg = compose(CFG_DIR, "train_binary_class_clf",
                  ["networks=clip_convnexttiny_bert_pixels", "tokenizer=bert_clinical_seqlen=77", "networks/dropout=dropout0",
                   "networks.image_encoder.micro_batch=4", "networks.image_encoder.image_size=[100,70]", "scheduler=warmup1_epo15",
                   "optimizer.config.learning_rate=1e-3", f"dataloader.train.batch_size={batch}", "dataset.config.synthetic_samples=12",
                   f"checkpoints.checkpoints_export_dir={tmp_path}/ckpt", f"base.tensorboard_export_dir={tmp_path}/tb"])
    loaders = train.build_loaders(cfg)
    assert loaders[0].kw["image_size"] == (100, 70)
    loader = SyntheticLoader(1, batch, seed=5, **{**loaders[0].kw, "vocab_size": 3000})
    assert next(iter(loader))["image"].shape == (batch, 1, 100, 70)
    torch.manual_seed(0)
    exp = create_experiment("classification")(config=cfg, train_dataloader=loader, valid_dataloader=None, test_dataloader=None, tokenizer=None)
    exp.scheduler.step()                                   # (the first epoch of the warm-up schedule runs at lr = 0: take the second one's rate)
    assert exp.optimizer.param_groups[0]["lr"] > 0

    def one_epoch(data):
        exp.train_dataloader = data
        before = {n: p.detach().clone() for n, p in exp.model.named_parameters() if p.requires_grad}
        loss = exp.train()
        assert math.isfinite(loss) and abs(loss - math.log(batch)) < 0.5, loss
        bad = [n for n, p in exp.model.named_parameters() if p.requires_grad and (p.grad is None or not torch.isfinite(p.grad).all())]
        assert not bad, bad[:5]
        # (BERT's pooler is not part of this model's function - the text feature is the EOS row - so its gradient is identically zero and its
        #  zero-initialised bias cannot move; every other trainable parameter has a non-zero gradient and moved)
        dead = [n for n, p in exp.model.named_parameters() if p.requires_grad and not p.grad.any()]
        assert all(".pooler." in n for n in dead), dead[:5]
        still = [n for n, p in exp.model.named_parameters() if p.requires_grad and n not in dead and torch.equal(p.detach(), before[n])]
        assert not still, still[:5]
        assert exp.optimizer.param_groups[0]["lr"] > 0
        return loss

    one_epoch(loader)
    b = synthetic_batch(batch, S=77, image_size=(100, 70), vocab_size=3000, seed=6)
    other = torch.rand(batch, 1, 77, 50, generator=torch.Generator().manual_seed(7))
    b["image"] = [b["image"][i] if i % 2 == 0 else other[i] for i in range(batch)]
    one_epoch([b])
