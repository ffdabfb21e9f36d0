"""The foreground prior of the ViT tower's patch dropout on the device (csrc/patch_dropout.hip, mmgclip/networks/vit.py):
`mmg_patch_foreground` against the CPU count of tests/patch_prior_ref.py and `mmg_patch_keep_indices_prior` against the numpy statement
(both exact), then the tower: kept sets, forward and backward against the fp32 reference of tests/patch_dropout_ref.py, and its exact
properties.  Every test here fails on the parent commit (no symbols, no arguments)."""
import numpy as np
import pytest
import torch

from mmgclip.kernels import PIXEL_KINDS
from mmgclip._hip import call, ptr, stream
from tests import augment_ref as AR
from tests import patch_dropout_ref as R
from tests import patch_prior_ref as PR
from tests.test_patch_dropout_gpu import _assert_same_gradients, _randomize, _rel

pytestmark = pytest.mark.gpu

BIG_SEED = 0x1234567890ABCDEF          # above 2^32: the high word enters the key
IDS = [7, 0, 2 ** 31 - 1, 3, 3]
HID = 768
T = 0.25
T_UP = float(np.nextafter(np.float32(T), np.float32(1)))


# ---- 1. the count: exact ----------------------------------------------------------------------------------------------------------------------
def _device_counts(dev, img, patch, threshold, geom):
    n, C, H, W = img.shape
    counts = torch.full((n, (H // patch) * (W // patch)), -7, device=dev, dtype=torch.int32)
    g = None if geom is None else torch.tensor(geom, dtype=torch.int32).to(dev)
    d = img.to(dev)
    call("mmg_patch_foreground", ptr(d), PIXEL_KINDS[img.dtype], n, C, H, W, patch, ptr(g), threshold, ptr(counts), stream())
    torch.cuda.synchronize()
    return counts.cpu()


def _pixels(dtype, shape, seed):
    """Values on both sides of the threshold: fp32 from {0, t, nextafter(t)} (so that > against >= is pinned), integers from the four
    values around t * 65535 (or t * 255) and the extremes - on which side each falls, the reference decides, with the division."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        return torch.tensor([0.0, T, T_UP])[torch.randint(0, 3, shape, generator=g)]
    top = 65535 if dtype == torch.uint16 else 255
    near = int(T * top)
    vals = torch.tensor([0, near - 1, near, near + 1, near + 2, top], dtype=torch.int32)
    return vals[torch.randint(0, 6, shape, generator=g)].to(dtype)


GEOMS = {"null": None, "identity": [0, 0, 0, 0], "flipx": [1, 0, 0, 0], "flipy": [2, 0, 0, 0], "flipxy": [3, 0, 0, 0], "shift": [0, -5, 7, 0],
         "flipxy_shift": [3, -5, 7, 0], "shift_out": [0, 70, 0, 0], "shift_out_x": [1, 0, -1040, 0]}


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("shape,dtype", [((3, 1, 64, 64), torch.float32), ((3, 3, 64, 64), torch.float32), ((3, 3, 64, 64), torch.uint8),
                                         ((2, 1, 70, 50), torch.uint8), ((2, 1, 70, 50), torch.uint16), ((2, 1, 70, 50), torch.float32),
                                         ((2, 3, 70, 51), torch.uint8), ((1, 1, 32, 1040), torch.uint16), ((1, 1, 32, 1040), torch.uint8)])
def test_counts_equal_the_reference(dev, shape, dtype, geom):
    """patch 16.  64 x 64: whole patches; 70 x 50 (and 51, odd uint8 rows): remainders ignored, rows at every alignment; 32 x 1040: more
    chunks than a workgroup has lanes.  Every flip, a shift, a shift of at least H (and of at least W): every count 0."""
    img = _pixels(dtype, shape, seed=shape[2] * 7 + shape[3])
    if dtype == torch.float32:
        img[0, 0, 3, 5] = img[-1, -1, 17, 33] = float("nan")
    rows = None if GEOMS[geom] is None else [GEOMS[geom]] * shape[0]
    ref = PR.foreground_counts(img, 16, T, rows)
    got = _device_counts(dev, img, 16, T, rows)
    assert torch.equal(got, ref), (got - ref).abs().max()
    if geom.startswith("shift_out"):
        assert int(ref.sum()) == 0
    else:
        assert int(ref.sum()) > 0 and int(ref.max()) < shape[1] * 256       # neither empty nor full: the threshold divides the pixels


def test_counts_per_image_geometry_and_every_uint16_value(dev):
    """Another row per image (flips, shifts of both signs), and all 65 536 uint16 values against three thresholds: the integer compare the
    kernel makes is the reference's float(r) / 65535 > t for every r."""
    img = _pixels(torch.uint8, (4, 1, 70, 50), seed=5)
    rows = [[0, 3, -9, 0], [1, -17, 20, 0], [2, 16, 16, 0], [3, 1, 1, 0]]
    assert torch.equal(_device_counts(dev, img, 16, T, rows), PR.foreground_counts(img, 16, T, rows))
    allv = torch.arange(65536, dtype=torch.int32).reshape(1, 1, 256, 256).to(torch.uint16)
    for t in (0.0, T, 0.7, float(np.nextafter(np.float32(1), np.float32(0)))):
        assert torch.equal(_device_counts(dev, allv, 16, t, None), PR.foreground_counts(allv, 16, t))
    assert torch.equal(_device_counts(dev, allv, 1, T, None), PR.foreground_counts(allv, 1, T))      # patch 1: the predicate per value


# ---- 2. the draw: exact ------------------------------------------------------------------------------------------------------------------------
def _device_draw(dev, seed, ids, counts, min_pixels, K):
    B, NP = counts.shape
    keep = torch.full((B, K), -7, device=dev, dtype=torch.int32)
    slot = torch.full((B, NP), -7, device=dev, dtype=torch.int32)
    nfg = torch.full((B,), -7, device=dev, dtype=torch.int32)
    idt = None if ids is None else torch.tensor(ids, dtype=torch.int64).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(dev)
    call("mmg_patch_keep_indices_prior", seed, ptr(idt), ptr(c), min_pixels, B, NP, K, ptr(keep), ptr(slot), ptr(nfg), stream())
    torch.cuda.synchronize()
    return keep.cpu(), slot.cpu(), nfg.cpu()


def _counts_with(nfg_rows, NP, seed, value=1):
    rng = np.random.default_rng(seed)
    counts = np.zeros((len(nfg_rows), NP), dtype=np.int32)
    for b, nfg in enumerate(nfg_rows):
        counts[b, rng.permutation(NP)[:nfg]] = value
    return counts


@pytest.mark.parametrize("NP,K", [(1, 1), (36, 18), (1024, 512), (1025, 3), (4096, 2048), (4097, 4000), (16384, 8192)])
def test_draw_equals_the_numpy_statement(dev, NP, K):
    """B = 5 under ids [7, 0, 2^31 - 1, 3, 3] and a seed above 2^32, at the sizes where the kernel changes the number of patches a thread
    owns; per row nfg in {0, 1, K-1, K, K+1, NP} (two launches of five rows), min_pixels 1 and 3."""
    clip = lambda v: [min(max(x, 0), NP) for x in v]                 # noqa: E731
    for rows, min_pixels in ((clip([0, 1, K - 1, K, K + 1]), 1), (clip([NP, K + 1, K, K - 1, NP // 2]), 3)):
        counts = _counts_with(rows, NP, seed=NP + min_pixels, value=min_pixels)
        if min_pixels > 1:
            counts[counts == 0] = np.random.default_rng(NP).integers(0, min_pixels, size=int((counts == 0).sum()))   # below the bar: background
        keep, slot, nfg = _device_draw(dev, BIG_SEED, IDS, counts, min_pixels, K)
        ref_keep, ref_slot, ref_nfg = PR.draw(BIG_SEED, IDS, counts, min_pixels, K)
        assert ref_nfg.tolist() == rows
        assert torch.equal(nfg, ref_nfg) and torch.equal(keep, ref_keep) and torch.equal(slot, ref_slot)


@pytest.mark.parametrize("NP,K", [(36, 18), (1025, 3), (4097, 4000), (16384, 8192)])
def test_draw_with_one_class_is_the_uniform_draw_bit_for_bit(dev, NP, K):
    keep0 = torch.full((5, K), -7, device=dev, dtype=torch.int32)
    slot0 = torch.full((5, NP), -7, device=dev, dtype=torch.int32)
    idt = torch.tensor(IDS, dtype=torch.int64).to(dev)
    call("mmg_patch_keep_indices", BIG_SEED, ptr(idt), 5, NP, K, ptr(keep0), ptr(slot0), stream())
    for fill, want in ((4, NP), (0, 0)):
        keep, slot, nfg = _device_draw(dev, BIG_SEED, IDS, np.full((5, NP), fill, dtype=np.int32), 1, K)
        assert torch.equal(keep, keep0.cpu()) and torch.equal(slot, slot0.cpu()) and nfg.tolist() == [want] * 5


def test_draw_without_ids_draws_under_the_position_and_without_n_foreground(dev):
    counts = _counts_with([0, 50, 98, 99, 150, 196], 196, seed=3)
    keep, slot, nfg = _device_draw(dev, 2 ** 62 - 1, None, counts, 1, 98)
    ref_keep, ref_slot, ref_nfg = PR.draw(2 ** 62 - 1, range(6), counts, 1, 98)
    assert torch.equal(keep, ref_keep) and torch.equal(slot, ref_slot) and torch.equal(nfg, ref_nfg)
    keep2 = torch.empty(6, 98, device=dev, dtype=torch.int32)
    slot2 = torch.empty(6, 196, device=dev, dtype=torch.int32)
    c = torch.from_numpy(counts).to(dev)
    call("mmg_patch_keep_indices_prior", 2 ** 62 - 1, None, ptr(c), 1, 6, 196, 98, ptr(keep2), ptr(slot2), None, stream())
    assert torch.equal(keep2.cpu(), ref_keep) and torch.equal(slot2.cpu(), ref_slot)


# ---- 3. the tower --------------------------------------------------------------------------------------------------------------------------------
SIZE, P36, HALF = 96, 36, 18           # 6 x 6 patches; the left half of every image exact black: 18 foreground patches (columns 3 .. 5)
N_IMG = 4
RIGHT = torch.tensor([p for p in range(P36) if p % 6 >= 3])


def _images(n, seed, dtype=torch.float32):
    img = torch.rand(n, 1, SIZE, SIZE, generator=torch.Generator().manual_seed(seed))
    img[..., :SIZE // 2] = 0.0
    if dtype == torch.uint16:
        return (img * 65535.0).round().to(torch.int32).to(torch.uint16)
    return img


def _make(dev, state, **kw):
    from mmgclip.networks.encoder import ViTB16Encoder
    kw.setdefault("micro_batch", 2)
    tower = ViTB16Encoder(image_size=SIZE, layers=2, **kw)
    tower.load_state_dict(state)
    return tower.to(dev)


def _spy(tower):
    """Record what the tower's prior draw returns."""
    seen, orig = [], tower._draw_patch_drop_prior

    def record(*a, **kw):
        out = orig(*a, **kw)
        seen.append((out[0].cpu(), out[1].cpu()))
        return out
    tower._draw_patch_drop_prior = record
    return seen


@pytest.fixture(scope="module")
def state():
    from mmgclip.networks.encoder import ViTB16Encoder
    torch.manual_seed(0)
    ref = ViTB16Encoder(image_size=SIZE, layers=2, micro_batch=2)
    _randomize(ref, 3)
    return {k: v.clone() for k, v in ref.state_dict().items()}


@pytest.fixture(scope="module")
def case(dev, state):
    """Rate 0.75 (K = 9 <= 18 foreground patches), 4 images in micro-batches of 2, one forward + backward under BIG_SEED: shared, never
    changed."""
    img = _images(N_IMG, 1).to(dev)
    wgt = torch.randn(N_IMG, HID, generator=torch.Generator().manual_seed(2)).to(dev)
    tower = _make(dev, state, patch_dropout=0.75, patch_prior="foreground")
    seen = _spy(tower)
    feat, grads = _run(tower, img, wgt, BIG_SEED)
    nfg, K = tower.last_patch_foreground
    return {"img": img, "wgt": wgt, "feat": feat, "grads": grads, "keep": seen[0][0], "slot": seen[0][1], "nfg": nfg.cpu(), "K": K}


def _run(tower, img, wgt, seed=None):
    tower.zero_grad(set_to_none=True)
    if seed is not None:
        tower.next_patch_drop_seed = seed
    feat = tower(img)
    (feat * wgt).sum().backward()
    return feat.detach().clone(), {n: p.grad.detach().clone() for n, p in tower.model.named_parameters()}


@pytest.mark.parametrize("rate,dtype,ids", [(0.75, torch.float32, None), (0.25, torch.uint16, [5, 9, 2])])
def test_tower_keeps_foreground_first_and_matches_the_reference(dev, state, rate, dtype, ids):
    """(i) at rate 0.75 (K = 9 <= 18) every kept patch is foreground, and keep is the statement applied to the reference counts; at 0.25
    (K = 27) all 18 foreground patches and 9 of the background.  (ii) forward and backward against the fp32 reference under the same indices,
    at the bars of tests/test_patch_dropout_gpu.py::_tower_against_reference (they are written inline there, so they are repeated here:
    features rel < 3e-2, cos > 0.999; gradients cos > 0.99, rel < 0.12).  (vii) last_patch_foreground is the reference's n_foreground."""
    n = 3
    img = _images(n, 9, dtype)
    wgt = torch.randn(n, HID, generator=torch.Generator().manual_seed(10))
    K = R.keep_count(P36, rate)
    counts = PR.foreground_counts(img, 16, 0.0)
    assert (counts[:, RIGHT] > 0).all() and int(counts.sum()) == int(counts[:, RIGHT].sum())
    ref_keep, ref_slot, ref_nfg = PR.draw(BIG_SEED, range(n) if ids is None else ids, counts, 1, K)
    assert ref_nfg.tolist() == [HALF] * n
    tower = _make(dev, state, patch_dropout=rate, patch_prior="foreground")
    seen = _spy(tower)
    tower.next_patch_drop_seed = BIG_SEED
    feat = tower(img.to(dev), sample_ids=ids)
    assert tower.next_patch_drop_seed is None and feat.shape == (n, HID)
    keep, slot = seen[0]
    assert torch.equal(keep, ref_keep) and torch.equal(slot, ref_slot)
    fg_kept = torch.isin(keep, RIGHT).sum(1)
    assert fg_kept.tolist() == [min(K, HALF)] * n
    nfg, k_used = tower.last_patch_foreground
    assert k_used == K and nfg.dtype == torch.int32 and nfg.is_cuda and torch.equal(nfg.cpu(), ref_nfg)
    sd = {k[len("model."):]: v.clone().requires_grad_(True) for k, v in state.items()}
    ref = R.vit_forward_kept(sd, AR.augmented_images(img), ref_keep)
    (ref * wgt).sum().backward()
    r, c = _rel(feat, ref)
    print(f"features: rel {r:.3e} cos {c:.6f}")
    assert r < 3e-2 and c > 0.999, (r, c)
    (feat * wgt.to(dev)).sum().backward()
    bad = {}
    for name, p in tower.model.named_parameters():
        if name.endswith("in_proj_bias"):
            continue        # its key third has an exactly-zero gradient (softmax shift invariance): noise only
        r, c = _rel(p.grad, sd[name].grad)
        print(f"{name}: rel {r:.3e} cos {c:.6f}")
        if not (c > 0.99 and r < 0.12):
            bad[name] = (r, c)
    assert not bad, f"{len(bad)} gradients off: {list(bad.items())[:8]}"


def test_counts_follow_the_forwards_flip(dev, state, case):
    """(iii) a spec that always flips over x, under a forced augmentation seed.  The flip puts the image's right (tissue) half on the
    canvas's left half, and a patch index is a canvas position: every kept patch lies in the canvas's left half - taken back through the
    flip, in the image's right half.  keep equals the statement on the reference counts under the same geometry rows."""
    from mmgclip import augment as A
    tower = _make(dev, state, patch_dropout=0.75, patch_prior="foreground", augment={"hflip": 1.0})
    geom, _ = A.draw(tower.augment, BIG_SEED + 1, range(N_IMG))
    assert geom == [[1, 0, 0, 0]] * N_IMG
    seen = _spy(tower)
    tower.next_augment_seed, tower.next_patch_drop_seed = BIG_SEED + 1, BIG_SEED
    with torch.no_grad():
        tower(case["img"])
    keep = seen[0][0]
    counts = PR.foreground_counts(case["img"].cpu(), 16, 0.0, geom)
    ref_keep, _, ref_nfg = PR.draw(BIG_SEED, range(N_IMG), counts, 1, case["K"])
    assert torch.equal(keep, ref_keep) and torch.equal(tower.last_patch_foreground[0].cpu(), ref_nfg)
    source_col = 5 - keep % 6                                        # the flip over x, per patch column
    assert ref_nfg.tolist() == [HALF] * N_IMG and (keep % 6 <= 2).all() and (source_col >= 3).all()
    assert (counts[:, RIGHT] == 0).all()                             # the canvas's right half is the image's black half
    assert not torch.equal(keep, case["keep"])


@pytest.mark.parametrize("micro_batch", [1, 3, 4])
def test_any_micro_batch_gives_the_same_bits(dev, state, case, micro_batch):
    """(iv) a row is a function of (seed, sample id, pixels, geometry row)."""
    tower = _make(dev, state, patch_dropout=0.75, patch_prior="foreground", micro_batch=micro_batch)
    seen = _spy(tower)
    feat, grads = _run(tower, case["img"], case["wgt"], BIG_SEED)
    assert torch.equal(seen[0][0], case["keep"]) and torch.equal(seen[0][1], case["slot"])
    assert torch.equal(feat, case["feat"])
    for n, g in grads.items():                                       # sums over rows in another grouping: the order noise of the fp32 atomics
        rel = float((g - case["grads"][n]).norm() / (case["grads"][n].norm() + 1e-30))
        assert rel < 1e-5, (micro_batch, n, rel)


@pytest.mark.parametrize("keep_last", ["1", "0"])
def test_checkpointed_recomputation_reads_the_same_indices(dev, state, case, monkeypatch, keep_last):
    """(iv) as test_patch_dropout_gpu's: the features' bits, gradients to the order noise of the fp32 atomics (1e-5)."""
    monkeypatch.setenv("MMG_CKPT_KEEP_LAST", keep_last)
    tower = _make(dev, state, patch_dropout=0.75, patch_prior="foreground", checkpoint=True)
    seen = _spy(tower)
    tower.next_patch_drop_seed = BIG_SEED
    feat = tower(case["img"])
    tower.next_patch_drop_seed = BIG_SEED + 5            # set between forward and backward: the recomputation must not draw again
    (feat * case["wgt"]).sum().backward()
    assert tower.next_patch_drop_seed == BIG_SEED + 5 and len(seen) == 1
    assert torch.equal(feat, case["feat"])
    for n, p in tower.model.named_parameters():
        gr = case["grads"][n]
        rel = float((p.grad - gr).norm() / (gr.norm() + 1e-30))
        assert rel < 1e-5, (keep_last, n, rel)


def test_uniform_prior_is_the_tower_without_the_arguments(dev, state, case):
    """(v) explicit defaults: the same calls, the same bits, under the same forced seed; nothing of the prior runs."""
    plain = _make(dev, state, patch_dropout=0.5)
    feat0, grads0 = _run(plain, case["img"], case["wgt"], BIG_SEED)
    explicit = _make(dev, state, patch_dropout=0.5, patch_prior="uniform", patch_threshold=0.0, patch_min_pixels=1, patch_dropout_eval=False)
    seen = _spy(explicit)
    feat, grads = _run(explicit, case["img"], case["wgt"], BIG_SEED)
    assert torch.equal(feat, feat0) and not seen and explicit.last_patch_foreground is None
    _assert_same_gradients(grads, grads0)
    ref_keep, _ = R.keep_indices(BIG_SEED, range(N_IMG), P36, 18)
    assert not torch.isin(torch.from_numpy(ref_keep), RIGHT).all()   # the uniform draw does keep black patches of these images
    fg = _make(dev, state, patch_dropout=0.5, patch_prior="foreground")
    assert not torch.equal(_run(fg, case["img"], case["wgt"], BIG_SEED)[0], feat0)


def test_eval_switch_makes_the_embedding_a_function_of_the_pixels(dev, state, case):
    """(vi) patch_dropout_eval: K patches under eval() too, drawn under seed 0 and sample id 0 for every image, no geometry, no seed taken
    from the training stream."""
    tower = _make(dev, state, patch_dropout=0.75, patch_prior="foreground", patch_dropout_eval=True, augment={"hflip": 1.0}).eval()
    seen = _spy(tower)
    tower.next_patch_drop_seed = 123
    with torch.no_grad():
        a = tower(case["img"])
    assert tower.next_patch_drop_seed == 123                         # not consumed
    counts = PR.foreground_counts(case["img"].cpu(), 16, 0.0)         # no flip: eval() does not augment
    ref_keep, _, ref_nfg = PR.draw(0, [0] * N_IMG, counts, 1, case["K"])
    assert torch.equal(seen[0][0], ref_keep) and torch.equal(tower.last_patch_foreground[0].cpu(), ref_nfg)
    perm = [2, 0, 3, 1]
    other = _make(dev, state, patch_dropout=0.75, patch_prior="foreground", patch_dropout_eval=True, micro_batch=3).eval()
    with torch.no_grad():
        other(case["img"][:1])                                       # what ran before does not matter
        b = other(case["img"][perm], sample_ids=[9, 8, 7, 6])
    for i, j in enumerate(perm):
        assert torch.equal(b[i], a[j]), (i, j)
    # the training stream's next draw is what it would have been without those eval() forwards
    from mmgclip.utils.global_utils import seeding
    seeding(21)
    fresh = _make(dev, state, patch_dropout=0.75, patch_prior="foreground", patch_dropout_eval=True)
    want = fresh._patch_drop_seeds.draw()
    seeding(21)
    used = _make(dev, state, patch_dropout=0.75, patch_prior="foreground", patch_dropout_eval=True).eval()
    with torch.no_grad():
        used(case["img"]), used(case["img"])
    assert used._patch_drop_seeds.draw() == want
    # with the switch false eval() sees every patch, as a tower without patch dropout
    off = _make(dev, state, patch_dropout=0.75, patch_prior="foreground").eval()
    plain = _make(dev, state).eval()
    with torch.no_grad():
        full = plain(case["img"])
        assert torch.equal(off(case["img"]), full) and off.last_patch_foreground is None
    assert not torch.equal(a, full)


def test_last_patch_foreground_reports_the_whole_input(dev, case):
    """(vii) n_foreground of every image of the input (not of the last micro-batch), with K: the share of tissue a rate drops is
    max(0, nfg - K) / nfg."""
    counts = PR.foreground_counts(case["img"].cpu(), 16, 0.0)
    _, _, ref_nfg = PR.draw(BIG_SEED, range(N_IMG), counts, 1, case["K"])
    assert case["K"] == 9 and case["nfg"].shape == (N_IMG,) and torch.equal(case["nfg"], ref_nfg) and ref_nfg.tolist() == [HALF] * N_IMG
    assert torch.isin(case["keep"], RIGHT).all()
