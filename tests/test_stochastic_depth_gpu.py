"""Stochastic depth of the ConvNeXt tower on the GPU: the two image-move kernels bit for bit against torch indexing, the tower against the
unchanged fp32 oracle, its invariances (micro-batch, checkpointing, list input, mixed sizes), no change where it is off, and the 8-bit backward.

The oracle needs no change: `E.convnext_forward` multiplies the branch by `sd["...layer_scale"]` with broadcasting, so the tests hand it an
effective entry [n, C, 1, 1] = layer_scale[None] * keep[b, :, None, None, None] / (1 - p_b) built by torch ops from the leaf - the leaf's gradient
is then the oracle's gradient under stochastic depth.  The masks come from oracle/dropout_oracle.py (the package's own restatement is held to it
in tests/test_stochastic_depth_cpu.py).  The forced seeds are found by a CPU search whose conditions are asserted; none is hard-coded."""
import numpy as np
import pytest
import torch

from oracle import dropout_oracle as D
from oracle import encoders_oracle as E
from tests.conftest import measured

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEPTHS = {"tiny": (3, 3, 9, 3), "base": (3, 3, 27, 3)}
RATE = 0.5


def _rel(a, b):
    a, b = a.detach().float().cpu().double().flatten(), b.detach().float().cpu().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30)), float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))


def _randomize(module, seed):
    """As tests/test_towers_gpu.py: layer scales of 0.3 .. 1 so that the blocks matter."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if n.endswith("layer_scale"):
                p.copy_(0.3 + 0.7 * torch.rand(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1 and n.endswith("weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() >= 2:
                p.mul_(2.5)


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(49, 96), (256, 96), (4, 768), (1, 1024)])
def test_image_swap_and_copy_bitwise(dev, rows, C):
    import ctypes

    from mmgclip import kernels as K
    n = 9
    x0 = torch.randn(n * rows, C, generator=torch.Generator().manual_seed(rows + C)).to(dev).to(BF)
    for pairs in ([], [(2, 7)], [(0, 5), (1, 8), (3, 6), (4, 7)]):
        flat = [0, 0] + [v for pr in pairs for v in pr]                 # (the table holds another block's pairs first: offset 1)
        devt = torch.tensor(flat, dtype=torch.int32, device=dev)
        host = (ctypes.c_int * len(flat))(*flat)
        x = x0.clone()
        assert K.image_swap_(x, n, devt, host, len(pairs), 1) is x
        idx = list(range(n))
        for i, j in pairs:
            idx[i], idx[j] = idx[j], idx[i]
        assert torch.equal(x.view(n, rows, C), x0.view(n, rows, C)[idx])
    for first, count in ((9, 0), (0, 0), (6, 3), (0, 3), (2, 3)):
        dst0 = torch.full_like(x0, 7.0)
        dst = dst0.clone()
        K.image_copy(x0, dst, n, first, count)
        want = dst0.view(n, rows, C).clone()
        want[first:first + count] = x0.view(n, rows, C)[first:first + count]
        assert torch.equal(dst.view(n, rows, C), want)
    a, b = torch.randn(C, device=dev), torch.randn(C, device=dev)
    assert torch.equal(K.scaled_add_(a.clone(), b, 2.0), a + 2.0 * b)           # (doubling is exact: one rounding on either side)


def test_image_moves_reject_bad_arguments_without_a_launch(dev):
    import ctypes

    from mmgclip import kernels as K
    n, rows, C = 9, 4, 96
    x = torch.zeros(n * rows, C, device=dev, dtype=BF)

    def swap(pairs, t=x, n=n):
        return K.image_swap_(t, n, torch.tensor(pairs, dtype=torch.int32, device=dev), (ctypes.c_int * len(pairs))(*pairs), len(pairs) // 2)
    for pairs in ([0, 9], [-1, 2], [0, 5, 5, 6], [3, 3]):
        with pytest.raises(RuntimeError, match="mmg_image_swap"):
            swap(pairs)
    odd = torch.zeros(n * rows, 100, device=dev, dtype=BF)              # an unsupported width: rows of 200 bytes
    with pytest.raises(RuntimeError, match="multiple of 8"):
        swap([0, 5], odd)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        K.image_copy(odd, torch.zeros_like(odd), n, 0, 1)
    with pytest.raises(RuntimeError, match="not inside"):
        K.image_copy(x, torch.zeros_like(x), n, 7, 3)
    torch.cuda.synchronize()
    assert not x.any()


# ---- the forced seed and the oracle -----------------------------------------------------------------------------------------------------
def _rates(variant):
    B = sum(DEPTHS[variant])
    return [RATE * b / (B - 1) for b in range(B)]


def _keep(variant, n, seed, ids=None):
    ids = np.arange(n) if ids is None else np.asarray(ids)
    return np.stack([D.keep_mask(ids, p, seed, b) for b, p in enumerate(_rates(variant))])


def _find_seed(variant, n, mb):
    """The first seed under which (a) some block keeps none of some micro-batch, (b) some block is dropped for the whole batch, (c) every stage
    has a block that keeps exactly one of the two samples of some micro-batch.  -> (seed, keep [B, n])."""
    depths = DEPTHS[variant]
    starts = np.cumsum((0,) + depths)
    for seed in range(20000):
        keep = _keep(variant, n, seed)
        per_mb = np.stack([keep[:, i:i + mb].sum(1) for i in range(0, n, mb)], 1)           # [B, micro-batches] kept counts
        a = bool((per_mb == 0).any())
        b = bool((keep.sum(1) == 0).any())
        c = all((per_mb[starts[s]:starts[s + 1]] == 1).any() for s in range(4))
        if a and b and c:
            assert (per_mb == 0).any() and (keep.sum(1) == 0).any() and keep[0].all()
            assert all((per_mb[starts[s]:starts[s + 1]] == 1).any() for s in range(4))
            return seed, keep
    raise AssertionError("no seed meets the conditions")


def _oracle(sd, img, wgt, variant, keep, **kw):
    """fp32 oracle under the keep matrix: -> (features [n, C], {name: gradient})."""
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    eff, b = dict(osd), 0
    for si, depth in enumerate(DEPTHS[variant]):
        for bi in range(depth):
            k = f"features.{1 + 2 * si}.{bi}.layer_scale"
            kb = torch.tensor(keep[b], dtype=torch.float32)
            eff[k] = osd[k][None] * kb[:, None, None, None] / (1.0 - _rates(variant)[b])
            b += 1
    pooled, _ = E.convnext_forward(eff, img, depths=DEPTHS[variant], **kw)
    (pooled.flatten(1) * wgt).sum().backward()
    return pooled.flatten(1).detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in osd.items()}


def _tower(variant, state, dev, **kw):
    from mmgclip.networks.encoder import ConvNextBaseEncoder, ConvNextTinyEncoder
    tower = (ConvNextTinyEncoder if variant == "tiny" else ConvNextBaseEncoder)(**kw)
    tower.load_state_dict(state)
    return tower.to(dev)


def _run(tower, img, wgt, seed, **fw):
    """One training-mode forward + backward under the forced seed -> (features, {name: gradient}), on the CPU."""
    tower.zero_grad(set_to_none=True)
    tower.next_drop_seed = seed
    feat = tower(img, **fw)
    assert tower.next_drop_seed is None                         # the forced seed was consumed: stochastic depth acted
    (feat * wgt.to(feat.device)).sum().backward()
    torch.cuda.synchronize()
    return feat.detach().float().cpu(), {n: p.grad.detach().float().cpu().clone() for n, p in tower.model.named_parameters()}


def _dropped_blocks(variant, keep):
    """Parameter-name prefixes of the blocks that no sample of the batch passes through."""
    out, b = [], 0
    for si, depth in enumerate(DEPTHS[variant]):
        for bi in range(depth):
            if not keep[b].any():
                out.append(f"features.{1 + 2 * si}.{bi}.")
            b += 1
    return out


@pytest.fixture(scope="module")
def tiny(dev):
    """tiny, 64 x 64, n = 6 in micro-batches of 2, rate 0.5: the state, the inputs, the forced seed, the oracle's and the device's results -
    computed once, shared by the tests below, never modified."""
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    torch.manual_seed(0)
    ref = ConvNextTinyEncoder(micro_batch=2, stochastic_depth_prob=RATE)
    _randomize(ref, 1)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    sd = {k[len("model."):]: v.clone() for k, v in state.items()}
    img = torch.rand(6, 1, 64, 64, generator=torch.Generator().manual_seed(2))
    wgt = torch.randn(6, 768, generator=torch.Generator().manual_seed(3))
    seed, keep = _find_seed("tiny", 6, 2)
    ofeat, ograd = _oracle(sd, img, wgt, "tiny", keep)
    tower = _tower("tiny", state, dev, micro_batch=2, stochastic_depth_prob=RATE)
    feat, grad = _run(tower, img.to(dev), wgt, seed)
    return dict(state=state, img=img, wgt=wgt, seed=seed, keep=keep, ofeat=ofeat, ograd=ograd, feat=feat, grad=grad, tower=tower)


# ---- 2. the tower against the fp32 oracle ------------------------------------------------------------------------------------------------
def test_tower_matches_the_oracle_under_the_same_masks(tiny):
    """Bars: those of tests/test_towers_gpu.py::test_convnext_tower_forward_backward (features rel < 1.5e-2, cos > 0.9999; every gradient
    rel < 4e-2, cos > 0.999).  Where the oracle's gradient is exactly zero - a block dropped for the whole batch - the device's is exactly zero."""
    r, c = _rel(tiny["feat"], tiny["ofeat"])
    print("stochastic depth, tiny: seed", tiny["seed"], "kept per block", tiny["keep"].sum(1).tolist(), "features", r, c)
    assert r < 1.5e-2 and c > 0.9999, (r, c)
    worst, zeros = {}, 0
    for name, g in tiny["grad"].items():
        og = tiny["ograd"][name]
        if not og.any():
            assert not g.any(), name
            zeros += 1
            continue
        worst[name] = _rel(g, og)
    dropped = _dropped_blocks("tiny", tiny["keep"])
    assert dropped and zeros == 9 * len(dropped)                # (a CNBlock has nine parameter tensors)
    assert all(not tiny["ograd"][n].any() for n in tiny["ograd"] if any(n.startswith(d) for d in dropped))
    measured("convnext_stochastic_depth", variant="tiny", seed=tiny["seed"], feat_rel=r, feat_cos=c,
             grad_rel_max=max(v[0] for v in worst.values()), grad_cos_min=min(v[1] for v in worst.values()))
    print("gradients: rel max", max(v[0] for v in worst.values()), "cos min", min(v[1] for v in worst.values()))
    bad = {k: v for k, v in worst.items() if not (v[1] > 0.999 and v[0] < 4e-2)}
    assert not bad, f"{len(bad)} of {len(worst)} gradients off: {list(bad.items())[:8]}"


@pytest.fixture(scope="module")
def base_fp8(dev):
    """base, 64 x 64, n = 4 in micro-batches of 2, fp8 from C = 128, rate 0.5: state, inputs, forced seed (shared by cases 2 and 5)."""
    from mmgclip.networks.encoder import ConvNextBaseEncoder
    torch.manual_seed(0)
    ref = ConvNextBaseEncoder(micro_batch=2, fp8=True, stochastic_depth_prob=RATE)
    _randomize(ref, 1)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    img = torch.rand(4, 1, 64, 64, generator=torch.Generator().manual_seed(2))
    wgt = torch.randn(4, 1024, generator=torch.Generator().manual_seed(3))
    seed, keep = _find_seed("base", 4, 2)
    return dict(state=state, img=img, wgt=wgt, seed=seed, keep=keep, feat={})


def test_fp8_tower_matches_the_fp8_oracle_under_the_same_masks(dev, base_fp8, monkeypatch):
    """e4m3 forward in all 36 blocks, bf16 backward (MMG_FP8_BWD=0).  Bars: the all-blocks branch of
    tests/test_towers_gpu.py::test_convnext_fp8_forward_matches_the_fp8_oracle (features rel < 0.1, cos > 0.995; gradients rel < 0.25, cos > 0.975)."""
    monkeypatch.setenv("MMG_FP8_BWD", "0")
    c = base_fp8
    sd = {k[len("model."):]: v.clone() for k, v in c["state"].items()}
    ofeat, ograd = _oracle(sd, c["img"], c["wgt"], "base", c["keep"], fp8_min_channels=128)
    tower = _tower("base", c["state"], dev, micro_batch=2, fp8=True, stochastic_depth_prob=RATE)
    tower.fp8_min_channels = 128
    feat, grad = _run(tower, c["img"].to(dev), c["wgt"], c["seed"])
    assert all(p.kind == "fp8" for p in tower.plan) and not tower.fp8_bwd_now
    c["feat"]["bf16_bwd"] = feat
    r, cs = _rel(feat, ofeat)
    print("stochastic depth, base fp8: seed", c["seed"], "kept per block", c["keep"].sum(1).tolist(), "features", r, cs)
    assert r < 0.1 and cs > 0.995, (r, cs)
    worst = {}
    for name, g in grad.items():
        if not ograd[name].any():
            assert not g.any(), name
            continue
        worst[name] = _rel(g, ograd[name])
    assert _dropped_blocks("base", c["keep"])
    measured("convnext_stochastic_depth", variant="base_fp8", seed=c["seed"], feat_rel=r, feat_cos=cs,
             grad_rel_max=max(v[0] for v in worst.values()), grad_cos_min=min(v[1] for v in worst.values()))
    print("gradients: rel max", max(v[0] for v in worst.values()), "cos min", min(v[1] for v in worst.values()))
    bad = {k: v for k, v in worst.items() if not (v[1] > 0.975 and v[0] < 0.25)}
    assert not bad, f"{len(bad)} of {len(worst)} gradients off: {list(bad.items())[:8]}"


# ---- 5. the 8-bit backward ------------------------------------------------------------------------------------------------------------
def test_fp8_backward_with_stochastic_depth(dev, base_fp8, monkeypatch):
    """Default MMG_FP8_BWD (the e5m2 backward runs): finite gradients, exact zeros for the blocks nobody passed through, and the forward's
    bits are those of the bf16-backward run above."""
    monkeypatch.delenv("MMG_FP8_BWD", raising=False)
    c = base_fp8
    tower = _tower("base", c["state"], dev, micro_batch=2, fp8=True, stochastic_depth_prob=RATE)
    tower.fp8_min_channels = 128
    feat, grad = _run(tower, c["img"].to(dev), c["wgt"], c["seed"])
    assert tower.fp8_bwd_now and all(p.fp8_bwd_weights for p in tower.plan)
    assert all(torch.isfinite(g).all() for g in grad.values())
    dropped = _dropped_blocks("base", c["keep"])
    assert dropped
    for name, g in grad.items():
        if any(name.startswith(d) for d in dropped):
            assert not g.any(), name
    if "bf16_bwd" not in c["feat"]:                             # (run alone: make the reference forward here)
        monkeypatch.setenv("MMG_FP8_BWD", "0")
        other = _tower("base", c["state"], dev, micro_batch=2, fp8=True, stochastic_depth_prob=RATE)
        other.fp8_min_channels = 128
        c["feat"]["bf16_bwd"] = _run(other, c["img"].to(dev), c["wgt"], c["seed"])[0]
    assert torch.equal(feat, c["feat"]["bf16_bwd"])


# ---- 3. invariances -------------------------------------------------------------------------------------------------------------------
def _same(a, b, rel, cos=None):
    if not b.any():
        assert not a.any()
        return
    r, c = _rel(a, b)
    assert r < rel and (cos is None or c > cos), (r, c)


def test_masks_do_not_depend_on_the_micro_batch(dev, tiny):
    """micro_batch 6 against 2: other kernel shapes, the same samples dropped.  Bar: tests/test_towers_gpu.py:90 (rel < 2e-2, cos > 0.9995)."""
    tower = _tower("tiny", tiny["state"], dev, micro_batch=6, stochastic_depth_prob=RATE)
    feat, grad = _run(tower, tiny["img"].to(dev), tiny["wgt"], tiny["seed"])
    _same(feat, tiny["feat"], 2e-2, 0.9995)
    for n, g in grad.items():
        _same(g, tiny["grad"][n], 2e-2, 0.9995)


def test_checkpointed_recomputation_reuses_the_schedule(dev, tiny):
    """checkpoint=True against False, as closely as test_convnext_gradient_checkpointing_equals_plain_backward holds them: features
    rel < 1e-5, gradients rel < 2e-3 (the order of fp32 atomics)."""
    tower = _tower("tiny", tiny["state"], dev, micro_batch=2, checkpoint=True, stochastic_depth_prob=RATE)
    feat, grad = _run(tower, tiny["img"].to(dev), tiny["wgt"], tiny["seed"])
    _same(feat, tiny["feat"], 1e-5)
    for n, g in grad.items():
        _same(g, tiny["grad"][n], 2e-3)


def test_list_input_equals_the_tensor_bitwise(dev, tiny):
    tower = tiny["tower"]
    tower.next_drop_seed = tiny["seed"]
    with torch.no_grad():                                       # (stochastic depth acts with or without gradients)
        feat = tower([t for t in tiny["img"].to(dev)])
    assert tower.next_drop_seed is None
    assert torch.equal(feat.float().cpu(), tiny["feat"])


def test_mixed_sizes_equal_each_size_alone_bitwise(dev, tiny):
    """Two sizes interleaved in one list against each size run alone under the sample ids it had in the list: per image, the same bits."""
    tower = tiny["tower"]
    g = torch.Generator().manual_seed(9)
    imgs = [torch.rand(1, *((64, 64) if i % 2 == 0 else (96, 64)), generator=g).to(dev) for i in range(6)]
    seed = tiny["seed"]
    with torch.no_grad():
        tower.next_drop_seed = seed
        mixed = tower(imgs)
        for ids in ([0, 2, 4], [1, 3, 5]):
            tower.next_drop_seed = seed
            alone = tower([imgs[i] for i in ids], sample_ids=ids)
            assert torch.equal(alone, mixed[ids])
    keep = _keep("tiny", 6, seed)
    assert (keep[:, [0, 2, 4]] != keep[:, [1, 3, 5]]).any()     # (the two groups really draw different masks)


# ---- 4. no change where it is off -------------------------------------------------------------------------------------------------------
def test_eval_and_rate_zero_are_the_tower_without_stochastic_depth(dev, tiny):
    img = tiny["img"].to(dev)
    plain = _tower("tiny", tiny["state"], dev, micro_batch=2)
    assert plain.stochastic_depth_prob == 0.0
    with torch.no_grad():
        want_eval = plain.eval()(img)
    tower = _tower("tiny", tiny["state"], dev, micro_batch=2, stochastic_depth_prob=RATE)
    with torch.no_grad():
        assert torch.equal(tower.eval()(img), want_eval)
    tower.train()
    _, grad = _run(tower, img, tiny["wgt"], tiny["seed"])       # a training step with stochastic depth builds the scaled working copies ...
    with torch.no_grad():
        assert torch.equal(tower.eval()(img), want_eval)        # ... which eval() must not read
    # and in train() a rate of 0 takes the path without it: no seed is drawn or consumed, same bits as the plain tower
    plain.train()
    plain.next_drop_seed = 123
    tower.train()
    tower.next_drop_seed = tiny["seed"]
    with torch.no_grad():
        assert torch.equal(plain(img), want_eval) and plain.next_drop_seed == 123
        assert not torch.equal(tower(img), want_eval)


# ---- 6. the depthwise convolution's by-image branch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 9, 17])
def test_dwconv7_matrix_core_kernel_by_image(dev, n, monkeypatch):
    """csrc/dwconv7_mfma.hip hands whole images to the XCD groups from n = 8 on (`by_image`), and with stochastic depth every n_k occurs:
    n = 8, 9 and 17 (n % 8 != 0: the groups own different numbers of images) on a 96 x 100 map (6 x 7 tiles, the last column partial), C = 96,
    forward and flip + add, against torch's fp32 convolution on bf16-rounded inputs and against the VALU kernels.  Bars: those of
    tests/test_kernels_gpu.py::test_dwconv7_matrix_core_kernel."""
    import torch.nn.functional as F

    from mmgclip import kernels as K

    def close(a, b, rtol, atol):
        np.testing.assert_allclose(a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy(), rtol=rtol, atol=atol)

    def r(shape, seed, scale=1.0):
        return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)
    H, W, C = 96, 100, 96
    assert K.dwconv_mfma_pays(n, H, W, C, False)                # the tower takes this kernel at this shape
    x = r((n, H, W, C), 16).to(BF)
    w, b = r((C, 1, 7, 7), 17, 0.1), r((C,), 18)
    w49 = w.reshape(C, 49).t().contiguous()
    monkeypatch.setenv("MMG_DWCONV_MFMA", "1")
    y = K.dwconv7(x.reshape(-1, C), w49, b, n, H, W, C)
    wq = w.to(BF).float()
    xf = x.float().permute(0, 3, 1, 2)
    close(y.reshape(n, H, W, C), F.conv2d(xf, wq, b, padding=3, groups=C).permute(0, 2, 3, 1), 5e-3, 1e-2)
    close(y.reshape(n, H, W, C), F.conv2d(xf, w, b, padding=3, groups=C).permute(0, 2, 3, 1), 1e-2, 2e-2)
    dy = r((n, H, W, C), 19).to(BF)
    res = r((n * H * W, C), 20).to(BF)
    dx = K.dwconv7(dy.reshape(-1, C), w49, None, n, H, W, C, add=res, flip=True)
    dref = F.conv_transpose2d(dy.float().permute(0, 3, 1, 2), wq, None, padding=3, groups=C).permute(0, 2, 3, 1)
    close(dx.reshape(n, H, W, C), dref + res.float().reshape(n, H, W, C), 1e-2, 3e-2)
    monkeypatch.setenv("MMG_DWCONV_MFMA", "0")
    close(y, K.dwconv7(x.reshape(-1, C), w49, b, n, H, W, C), 1e-2, 2e-2)
    close(dx, K.dwconv7(dy.reshape(-1, C), w49, None, n, H, W, C, add=res, flip=True), 1e-2, 3e-2)
