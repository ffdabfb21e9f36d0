"""Patch dropout of the ViT tower on the device (csrc/patch_dropout.hip, mmgclip/networks/vit.py): the draw against its numpy statement,
the row movers against torch indexing and against the full-sequence assemble kernels (exact), the tower against the CPU reference
tests/patch_dropout_ref.py at the bars of test_vit_tower_forward_backward, and the tower's exact properties.  Every test here fails on the
parent commit (no symbols, no argument)."""
import numpy as np
import pytest
import torch

from mmgclip import augment as A
from mmgclip._hip import call, ptr, stream
from tests import augment_ref as AR
from tests import patch_dropout_ref as R

pytestmark = pytest.mark.gpu

BIG_SEED = 0x1234567890ABCDEF          # above 2^32: the high word enters the key
H = 768


def _rel(a, b):
    a, b = a.detach().float().cpu().double().flatten(), b.detach().float().cpu().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30)), float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))


def _randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1 and n.endswith("weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() >= 2:
                p.mul_(2.5)
        module.model.class_token.normal_(std=0.5, generator=g)


# ---- 1. the draw ----------------------------------------------------------------------------------------------------------------------------
def _device_draw(dev, seed, ids, B, P, K):
    keep = torch.full((B, K), -7, device=dev, dtype=torch.int32)
    slot = torch.full((B, P), -7, device=dev, dtype=torch.int32)
    idt = None if ids is None else torch.tensor(ids, dtype=torch.int64).to(dev)
    call("mmg_patch_keep_indices", seed, ptr(idt), B, P, K, ptr(keep), ptr(slot), stream())
    torch.cuda.synchronize()
    return keep.cpu(), slot.cpu()


@pytest.mark.parametrize("P,K", [(36, 18), (36, 1), (36, 36), (289, 216), (1024, 512), (1025, 3), (4096, 2048), (4097, 4000), (16384, 8192)])
def test_draw_equals_the_numpy_statement(dev, P, K):
    """B = 5 under ids [7, 0, 2^31 - 1, 3, 3] and a seed above 2^32.  (1024 | 1025, 4096 | 4097: where the kernel changes the number of patches
    a thread owns; 16384: all the LDS layout holds.)"""
    ids = [7, 0, 2 ** 31 - 1, 3, 3]
    keep, slot = _device_draw(dev, BIG_SEED, ids, 5, P, K)
    ref_keep, ref_slot = R.keep_indices(BIG_SEED, ids, P, K)
    assert torch.equal(keep, torch.from_numpy(ref_keep)) and torch.equal(slot, torch.from_numpy(ref_slot))


def test_draw_without_ids_draws_under_the_position(dev):
    keep, slot = _device_draw(dev, 2 ** 62 - 1, None, 6, 196, 98)
    ref_keep, ref_slot = R.keep_indices(2 ** 62 - 1, range(6), 196, 98)
    assert torch.equal(keep, torch.from_numpy(ref_keep)) and torch.equal(slot, torch.from_numpy(ref_slot))


# ---- 2. gather and assemble: exact -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,K", [(36, 18), (36, 36), (289, 216), (289, 289)])
def test_row_movers_equal_indexing_and_the_full_assemble_kernels(dev, P, K):
    B, Kp = 3, 256
    g = torch.Generator().manual_seed(P * 1000 + K)
    keep_np, slot_np = R.keep_indices(BIG_SEED, range(B), P, K)
    keep, slot = torch.from_numpy(keep_np).to(dev), torch.from_numpy(slot_np).to(dev)
    kl = torch.from_numpy(keep_np).long()
    rows = (torch.arange(B)[:, None] * P + kl).reshape(-1)                       # the kept rows of a [B*P, .] tensor

    p0 = torch.randn(B * P, Kp, generator=g).to(torch.bfloat16).to(dev)          # gather
    out = torch.empty(B * K, Kp, device=dev, dtype=torch.bfloat16)
    call("mmg_gather_patch_rows", ptr(p0), Kp, ptr(keep), ptr(out), B, P, K, Kp, stream())
    assert torch.equal(out.cpu(), p0.cpu()[rows])
    wide = torch.randn(B * P, Kp + 64, generator=g).to(torch.bfloat16).to(dev)   # a row stride above the width
    call("mmg_gather_patch_rows", ptr(wide), Kp + 64, ptr(keep), ptr(out), B, P, K, Kp, stream())
    assert torch.equal(out.cpu(), wide.cpu()[rows][:, :Kp])

    tok = torch.randn(B * P, H, generator=g).to(torch.bfloat16).to(dev)          # forward
    cls = torch.randn(H, generator=g).to(torch.bfloat16).to(dev)
    pos = torch.randn(1 + P, H, generator=g).to(torch.bfloat16).to(dev)
    full = torch.empty(B, 1 + P, H, device=dev, dtype=torch.bfloat16)
    call("mmg_vit_assemble_fwd", ptr(tok), ptr(cls), ptr(pos), ptr(full), B, 1 + P, H, stream())
    tok_kept = tok[rows.to(dev)].contiguous()
    x = torch.empty(B, 1 + K, H, device=dev, dtype=torch.bfloat16)
    call("mmg_vit_assemble_keep_fwd", ptr(tok_kept), ptr(cls), ptr(pos), ptr(keep), ptr(x), B, P, K, H, stream())
    seq = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + kl], 1)            # rows [0] + (1 + keep) of the full sequence
    assert torch.equal(x.cpu(), full.cpu()[torch.arange(B)[:, None], seq])

    gk = torch.randn(B, 1 + K, H, generator=g).to(torch.bfloat16)                # backward
    gfull = torch.zeros(B, 1 + P, H, dtype=torch.bfloat16)
    gfull[torch.arange(B)[:, None], seq] = gk
    dpos0, dcls0 = torch.randn(1 + P, H, generator=g), torch.randn(H, generator=g)
    dtok_f = torch.empty(B * P, H, device=dev, dtype=torch.bfloat16)
    dpos_f, dcls_f = dpos0.to(dev), dcls0.to(dev)
    gfull_dev = gfull.to(dev)
    call("mmg_vit_assemble_bwd", ptr(gfull_dev), ptr(dtok_f), ptr(dpos_f), ptr(dcls_f), B, 1 + P, H, stream())
    dtok = torch.full((B * K, H), 3.0, device=dev, dtype=torch.bfloat16)
    dpos, dcls = dpos0.to(dev), dcls0.to(dev)
    gk_dev = gk.to(dev)
    call("mmg_vit_assemble_keep_bwd", ptr(gk_dev), ptr(slot), ptr(dtok), ptr(dpos), ptr(dcls), B, P, K, H, stream())
    assert torch.equal(dtok.cpu(), dtok_f.cpu()[rows]) and torch.equal(dtok.cpu(), gk[:, 1:].reshape(B * K, H))
    assert torch.equal(dpos, dpos_f) and torch.equal(dcls, dcls_f)
    nobody = torch.from_numpy((slot_np < 0).all(0))                              # positions that no image kept stay as they were
    assert torch.equal(dpos.cpu()[1:][nobody], dpos0[1:][nobody])
    assert nobody.any() == (K < P)


# ---- 3. the tower against the reference ---------------------------------------------------------------------------------------------------
def _tower_against_reference(dev, image_size, layers, rate, n, ids=None, augment=None, seed_w=8):
    from mmgclip.networks.encoder import ViTB16Encoder
    torch.manual_seed(0)
    tower = ViTB16Encoder(image_size=image_size, layers=layers, micro_batch=2, patch_dropout=rate, augment=augment)
    _randomize(tower, seed_w)
    sd = {k[len("model."):]: v.clone() for k, v in tower.state_dict().items()}
    img = torch.rand(n, 1, image_size, image_size, generator=torch.Generator().manual_seed(9))
    wgt = torch.randn(n, H, generator=torch.Generator().manual_seed(10))
    P = (image_size // 16) ** 2
    K = R.keep_count(P, rate)
    keep, _ = R.keep_indices(BIG_SEED, range(n) if ids is None else ids, P, K)
    pre = img
    if augment is not None:
        geom, tone = A.draw(tower.augment, BIG_SEED + 1, range(n) if ids is None else ids)
        assert any(r[0] for r in geom) and not all(r[0] for r in geom)          # some images flipped, some not
        pre = AR.augmented_images(img, geom, tone)
        tower.next_augment_seed = BIG_SEED + 1
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = R.vit_forward_kept(osd, pre, keep)
    (ref * wgt).sum().backward()
    tower = tower.to(dev)
    tower.next_patch_drop_seed = BIG_SEED
    feat = tower(img.to(dev), sample_ids=ids)
    assert tower.next_patch_drop_seed is None and feat.shape == (n, H)
    r, c = _rel(feat, ref)
    print(f"features: rel {r:.3e} cos {c:.6f}")
    assert r < 3e-2 and c > 0.999, (r, c)
    (feat * wgt.to(dev)).sum().backward()
    bad = {}
    for name, p in tower.model.named_parameters():
        if name.endswith("in_proj_bias"):
            continue        # its key third has an exactly-zero gradient (softmax shift invariance): noise only
        r, c = _rel(p.grad, osd[name].grad)
        print(f"{name}: rel {r:.3e} cos {c:.6f}")
        if not (c > 0.99 and r < 0.12):
            bad[name] = (r, c)
    assert not bad, f"{len(bad)} gradients off: {list(bad.items())[:8]}"
    return K


@pytest.mark.parametrize("ids", [None, [5, 9, 2]])
def test_tower_forward_backward_on_the_kept_tokens(dev, ids):
    """96 x 96, 3 layers, rate 0.5, 3 images in micro-batches of 2: the second micro-batch starts at sample id 2."""
    assert _tower_against_reference(dev, 96, 3, 0.5, 3, ids=ids) == 18


@pytest.mark.parametrize("image_size,rate,s_eff", [(272, 0.25, 217), (368, 0.5, 265)])
def test_attention_path_follows_the_kept_length(dev, image_size, rate, s_eff):
    """272 at 0.25: S_eff = 217 tokens where the full sequence (290) would take the tiled backward; 368 at 0.5: S_eff = 265, the backward is
    tiled and the forward is not."""
    assert 1 + _tower_against_reference(dev, image_size, 2, rate, 2) == s_eff


def test_tower_with_augmentation_drops_after_the_flip(dev):
    _tower_against_reference(dev, 96, 2, 0.5, 4, augment={"hflip": 0.5})


# ---- 4. exact properties of the tower -------------------------------------------------------------------------------------------------------
N_IMG, SIZE, P36, K18 = 4, 96, 36, 18


@pytest.fixture(scope="module")
def case(dev):
    """A 2-layer tower at 96 x 96 with rate 0.5, 4 images in micro-batches of 2, one forward + backward under BIG_SEED: shared, never changed."""
    from mmgclip.networks.encoder import ViTB16Encoder
    torch.manual_seed(0)
    ref = ViTB16Encoder(image_size=SIZE, layers=2, micro_batch=2)
    _randomize(ref, 3)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    img = torch.rand(N_IMG, 1, SIZE, SIZE, generator=torch.Generator().manual_seed(1)).to(dev)
    wgt = torch.randn(N_IMG, H, generator=torch.Generator().manual_seed(2)).to(dev)
    feat, grads = _run(_make(dev, state, patch_dropout=0.5), img, wgt, BIG_SEED)
    return {"state": state, "img": img, "wgt": wgt, "feat": feat, "grads": grads}


def _make(dev, state, **kw):
    from mmgclip.networks.encoder import ViTB16Encoder
    tower = ViTB16Encoder(image_size=SIZE, layers=2, micro_batch=2, **kw)
    tower.load_state_dict(state)
    return tower.to(dev)


def _run(tower, img, wgt, seed=None):
    tower.zero_grad(set_to_none=True)
    if seed is not None:
        tower.next_patch_drop_seed = seed
    feat = tower(img)
    (feat * wgt).sum().backward()
    return feat.detach().clone(), {n: p.grad.detach().clone() for n, p in tower.model.named_parameters()}


def _assert_same_gradients(a, b):
    """The position and class-token gradients bit for bit: the assemble kernels write them with one writer per element, from the data
    gradient at the very END of the backward chain, so their bits certify every data gradient before them.  The other parameters' gradients
    are sums over rows that mmg_layernorm_bwd and the weight-gradient GEMMs take with fp32 atomics (csrc/norm_elementwise.hip,
    csrc/gemm_bf16.hip): two backward passes over the SAME bits differ there in the order of the additions (measured on this tower between two
    runs of identical inputs, on the launches of a tower without patch dropout: up to 1.2e-7 relative), so they are held to the order-noise
    bar of test_vit_gradient_checkpointing_equals_plain_backward, 1e-5."""
    gaps = {n: float((a[n] - b[n]).norm() / (b[n].norm() + 1e-30)) for n in b if not torch.equal(a[n], b[n])}
    print("gradients whose bits differ:", gaps)
    assert set(a) == set(b) and {"encoder.pos_embedding", "class_token"} <= set(b)
    bad = {n: r for n, r in gaps.items() if n in ("encoder.pos_embedding", "class_token") or not r < 1e-5}
    assert not bad, bad


def test_dropped_pixels_are_never_read(dev, case):
    keep, _ = R.keep_indices(BIG_SEED, range(N_IMG), P36, K18)
    other = case["img"].clone()
    noise = torch.rand(other.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    for b in range(N_IMG):
        for p in set(range(P36)) - set(keep[b].tolist()):
            y, x = p // 6 * 16, p % 6 * 16
            other[b, :, y:y + 16, x:x + 16] = noise[b, :, y:y + 16, x:x + 16]
    assert not torch.equal(other, case["img"])
    feat, grads = _run(_make(dev, case["state"], patch_dropout=0.5), other, case["wgt"], BIG_SEED)
    assert torch.equal(feat, case["feat"])
    _assert_same_gradients(grads, case["grads"])


def test_position_gradient_is_zero_where_no_image_kept_the_patch(dev, case):
    _, slot = R.keep_indices(BIG_SEED, range(N_IMG), P36, K18)
    nobody = torch.from_numpy((slot < 0).all(0))
    assert nobody.any() and not nobody.all()
    g = case["grads"]["encoder.pos_embedding"].cpu()[0]
    assert torch.equal(g[1:][nobody], torch.zeros(int(nobody.sum()), H))
    assert (g[1:][~nobody].abs().sum(1) > 0).all() and g[0].abs().sum() > 0


@pytest.mark.parametrize("keep_last", ["1", "0"])
def test_checkpointed_recomputation_reads_the_same_indices(dev, case, monkeypatch, keep_last):
    """As test_vit_gradient_checkpointing_equals_plain_backward: the features' bits, gradients to the order noise of the fp32 atomics."""
    monkeypatch.setenv("MMG_CKPT_KEEP_LAST", keep_last)
    tower = _make(dev, case["state"], patch_dropout=0.5, checkpoint=True)
    tower.next_patch_drop_seed = BIG_SEED
    feat = tower(case["img"])
    tower.next_patch_drop_seed = BIG_SEED + 5            # set between forward and backward: the recomputation must not draw again
    (feat * case["wgt"]).sum().backward()
    assert tower.next_patch_drop_seed == BIG_SEED + 5
    assert torch.equal(feat, case["feat"])
    for n, p in tower.model.named_parameters():
        gr = case["grads"][n]
        rel = float((p.grad - gr).norm() / (gr.norm() + 1e-30))
        assert rel < 1e-5, (keep_last, n, rel)


def test_rate_zero_and_eval_give_the_bits_of_a_tower_without_the_argument(dev, case):
    plain = _make(dev, case["state"])
    feat0, grads0 = _run(plain, case["img"], case["wgt"])
    assert not torch.equal(feat0, case["feat"])
    zero = _make(dev, case["state"], patch_dropout=0.0)
    zero.next_patch_drop_seed = 123                      # never consumed: no draw at rate 0
    feat, grads = _run(zero, case["img"], case["wgt"])
    assert zero.next_patch_drop_seed == 123 and torch.equal(feat, feat0)
    _assert_same_gradients(grads, grads0)
    half = _make(dev, case["state"], patch_dropout=0.5).eval()
    half.next_patch_drop_seed = 123
    with torch.no_grad():
        assert torch.equal(half(case["img"]), plain.eval()(case["img"]))
    assert half.next_patch_drop_seed == 123
    feat, _ = _run(half, case["img"], case["wgt"])       # eval() with a recorded backward: still every patch
    assert torch.equal(feat, feat0)
    half.train().patch_dropout = 0.0                     # reassigned between steps
    assert torch.equal(_run(half, case["img"], case["wgt"])[0], feat0)


def test_same_seed_agrees_and_fresh_seeds_differ(dev, case):
    tower = _make(dev, case["state"], patch_dropout=0.5)
    feat, grads = _run(tower, case["img"], case["wgt"], BIG_SEED)
    assert torch.equal(feat, case["feat"])
    _assert_same_gradients(grads, case["grads"])
    seen = []
    spy = tower._draw_patch_drop

    def record(count, sample_ids, device):
        out = spy(count, sample_ids, device)
        seen.append(out[0].cpu())
        return out
    tower._draw_patch_drop = record
    with torch.no_grad():
        a, b = tower(case["img"]), tower(case["img"])    # no forced seed: the tower's own stream, two draws
    assert len(seen) == 2 and seen[0].shape == (N_IMG, K18) and not torch.equal(seen[0], seen[1])
    assert not torch.equal(a, b)
    with pytest.raises(ValueError):
        tower(case["img"], sample_ids=[0, 1])
