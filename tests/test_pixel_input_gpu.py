"""Raw 8/16-bit pixels and seeded augmentation in the stem's patchify (csrc/pixel_input.hip, mmgclip/augment.py) on the device.
Every comparison is torch.equal - bit for bit - unless it says otherwise: against the fp32 kernel (`mmg_patchify`, unchanged) and against
tests/augment_ref.py, the arithmetic in torch fp32 on the CPU.  Every test here fails on the parent commit (no `geom` / `tone` / `augment`
keywords, no integer input without a conversion)."""
import os

import numpy as np
import pytest
import torch

from mmgclip import augment as A
from tests import augment_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "mmg-clip_amd", "configs")
SEED = 90210
EVERY_KNOB = A.AugmentSpec(hflip=0.5, vflip=0.5, max_shift=8, gain=(0.8, 1.2), offset=(-0.1, 0.1))


def _rel(a, b):
    a, b = a.detach().float().cpu().double().flatten(), b.detach().float().cpu().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _tables(geom, tone, dev):
    return (None if geom is None else torch.tensor(geom, dtype=torch.int32, device=dev),
            None if tone is None else torch.tensor(tone, dtype=torch.float32, device=dev))


def _as_kind(x, kind):
    """fp32 draws in [0, 1] -> the source kind under test."""
    from mmgclip.dataset.synthetic import as_pixel_dtype
    return as_pixel_dtype(x, kind)


def _three_way(dev, img, P, Kp, scale16):
    """K.patchify on the integers == K.patchify on v / top in fp32 (the old kernel) == the CPU reference."""
    from mmgclip import kernels as K
    top = R.KIND_DIV[img.dtype]
    as_float = img.to(torch.int32).to(torch.float32) / top
    new = K.patchify(img.to(dev), P, Kp, scale16).cpu()
    old = K.patchify(as_float.to(dev), P, Kp, scale16).cpu()
    ref = R.patch_rows(img, P, Kp, scale16)
    assert new.dtype == torch.bfloat16 and new.shape == ref.shape
    assert torch.equal(new, old), "integer path differs from the fp32 kernel"
    assert torch.equal(new, ref), "integer path differs from the CPU reference"
    k = P * P * img.shape[1]
    assert (new[:, k:] == 0).all()


# ---- 1. the integer paths, exhaustively ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Kp", [(4, 32), (16, 256)])          # the 1 x 4 fast path; the generic kernel as the ViT uses it
@pytest.mark.parametrize("scale16", [True, False])
def test_every_16_bit_value(dev, P, Kp, scale16):
    v = torch.randperm(65536, generator=torch.Generator().manual_seed(3)).to(torch.int32).to(torch.uint16).reshape(1, 1, 256, 256)
    assert len(set(v.to(torch.int32).flatten().tolist())) == 65536
    _three_way(dev, v, P, Kp, scale16)


@pytest.mark.parametrize("P,Kp", [(4, 32), (16, 256)])
@pytest.mark.parametrize("scale16", [True, False])
def test_every_8_bit_value(dev, P, Kp, scale16):
    v = (torch.randperm(1024, generator=torch.Generator().manual_seed(4)) % 256).to(torch.uint8).reshape(1, 1, 32, 32)
    assert sorted(v.flatten().tolist()) == sorted(list(range(256)) * 4)
    _three_way(dev, v, P, Kp, scale16)


@pytest.mark.parametrize("kind", ["uint16", "uint8"])
def test_generic_path_three_channels(dev, kind):
    """Cin = 3, Kp = 64: plain, and (37 x 50, no multiple of 4) with flips, an odd shift and tone."""
    from mmgclip import kernels as K
    img = _as_kind(torch.rand(2, 3, 32, 48, generator=torch.Generator().manual_seed(5)), kind)
    _three_way(dev, img, 4, 64, True)
    img = _as_kind(torch.rand(2, 3, 37, 50, generator=torch.Generator().manual_seed(6)), kind)
    geom, tone = [[3, -5, 3, 0], [1, 2, -7, 0]], [[1.0, 0.0], [1.6, -0.2]]
    for scale16 in (True, False):
        got = K.patchify(img.to(dev), 4, 64, scale16, *_tables(geom, tone, dev)).cpu()
        assert torch.equal(got, R.patch_rows(img, 4, 64, scale16, geom, tone))
        assert (got[:, 48:] == 0).all()


# ---- 2. geometry and tone ---------------------------------------------------------------------------------------------------------------
GEOM5 = [[0, 0, 0, 0], [3, 0, 0, 0], [0, -5, 3, 0], [0, 40, 0, 0], [1, 2, -7, 0]]
TONE5 = [[1.0, 0.0], [1.0, 0.0], [1.0, 0.0], [1.0, 0.0], [1.6, -0.2]]


@pytest.mark.parametrize("kind", ["uint16", "uint8", "float32"])
def test_geometry_and_tone_at_a_ragged_size(dev, kind):
    """[5, 1, 37, 50] on the 1 x 4 fast path: identity; flip x + flip y (over the FULL 50 columns: the two dropped ones are the source's
    first two); an odd shift (misaligned reads); everything fill; flip x + shift + a tone that clamps at both ends."""
    from mmgclip import kernels as K
    img = _as_kind(torch.rand(5, 1, 37, 50, generator=torch.Generator().manual_seed(7)), kind)
    x01 = R.augmented_images(img, GEOM5, TONE5)
    assert (x01[4] == 0).any() and (x01[4] == 1).any()                  # the tone clamps at both ends
    assert (x01[3] == 0).all()                                          # (40, 0): everything fill
    flipped = R.unit_pixels(img[1:2]).flip(-1).flip(-2)
    assert torch.equal(x01[1:2], flipped)                               # the canvas keeps source columns 49 .. 2: 0 and 1 are the dropped ones
    for scale16 in (True, False):
        got = K.patchify(img.to(dev), 4, 32, scale16, *_tables(GEOM5, TONE5, dev)).cpu()
        ref = R.patch_rows(img, 4, 32, scale16, GEOM5, TONE5)
        assert got.shape == (5 * 9 * 12, 32)
        for i in range(5):
            assert torch.equal(got[i * 108:(i + 1) * 108], ref[i * 108:(i + 1) * 108]), (i, scale16)
        assert (got[:, 16:] == 0).all()


@pytest.mark.parametrize("kind", ["uint16", "uint8", "float32"])
def test_geometry_and_tone_on_the_aligned_branch(dev, kind):
    """[2, 1, 32, 64] with shifts that are multiples of 8: every in-image read of the fast path is one wide load, flipped or not.  Also each
    table alone (the other NULL)."""
    from mmgclip import kernels as K
    img = _as_kind(torch.rand(2, 1, 32, 64, generator=torch.Generator().manual_seed(8)), kind)
    geom, tone = [[0, 8, -16, 0], [3, -8, 8, 0]], [[1.0, 0.0], [1.1, 0.02]]
    for g, t in ((geom, tone), (geom, None), (None, tone)):
        for scale16 in (True, False):
            got = K.patchify(img.to(dev), 4, 32, scale16, *_tables(g, t, dev)).cpu()
            assert torch.equal(got, R.patch_rows(img, 4, 32, scale16, g, t)), (g is None, t is None, scale16)
            assert (got[:, 16:] == 0).all()


def test_float_input_without_tables_still_takes_the_old_entry(dev):
    """fp32 with identity rows through mmg_patchify_aug == fp32 without tables through mmg_patchify."""
    from mmgclip import kernels as K
    img = torch.rand(2, 1, 40, 36, generator=torch.Generator().manual_seed(9)).to(dev)
    plain = K.patchify(img, 4, 32, True)
    ident = K.patchify(img, 4, 32, True, *_tables([[0, 0, 0, 0]] * 2, [[1.0, 0.0]] * 2, dev))
    assert torch.equal(plain, ident)
    with pytest.raises(TypeError):
        K.patchify(img.to(torch.float16), 4, 32, True)


# ---- 3. the ConvNeXt tower --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tower_case(dev):
    """uint16 [4, 1, 100, 70]; the reference: the same weights without `augment`, fed the fp32 images the CPU reference makes from draw's rows."""
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    torch.manual_seed(0)
    img = _as_kind(torch.rand(4, 1, 100, 70, generator=torch.Generator().manual_seed(1)), "uint16")
    wgt = torch.randn(4, 768, generator=torch.Generator().manual_seed(2)).to(dev)
    geom, tone = A.draw(EVERY_KNOB, SEED, range(4))
    assert any(r[0] for r in geom) and any(r[1] or r[2] for r in geom)
    pre = R.augmented_images(img, geom, tone)
    ref = ConvNextTinyEncoder(micro_batch=4)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    ref = ref.to(dev)
    feat = ref(pre.to(dev))
    (feat * wgt).sum().backward()
    grads = {n: p.grad.detach().clone() for n, p in ref.model.named_parameters()}
    return img, wgt, state, feat.detach().clone(), grads


def _augmented_tower(dev, state, **kw):
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    tower = ConvNextTinyEncoder(augment=EVERY_KNOB, **kw)
    tower.load_state_dict(state)
    return tower.to(dev)


@pytest.mark.parametrize("mb", [4, 2, 3])
def test_tower_on_raw_pixels_with_augmentation(dev, tower_case, mb):
    """Features bit-identical to the un-augmented tower on the pre-augmented fp32 images, every gradient rel < 2e-3 (the bar of
    test_ragged_size_micro_batch_independence: order of fp32 atomics) - in one micro-batch of 4, two of 2, and 3 + 1."""
    img, wgt, state, feat_ref, grads_ref = tower_case
    tower = _augmented_tower(dev, state, micro_batch=mb)
    tower.next_augment_seed = SEED
    feat = tower(img.to(dev))
    assert tower.next_augment_seed is None
    (feat * wgt).sum().backward()
    assert torch.isfinite(feat).all() and torch.equal(feat, feat_ref)
    for n, p in tower.model.named_parameters():
        assert _rel(p.grad, grads_ref[n]) < 2e-3, (mb, n)
    tower.next_augment_seed = SEED + 1                   # another seed: other pixels
    with torch.no_grad():
        assert not torch.equal(tower(img.to(dev)), feat_ref)


@pytest.mark.parametrize("keep_last", ["0", "1"])
def test_tower_checkpointed_recomputation_reads_the_same_rows(dev, tower_case, monkeypatch, keep_last):
    """checkpoint=True, micro-batches of 2: features rel < 1e-5 (as test_ragged_size_gradient_checkpointing_equals_plain_backward has it),
    every gradient rel < 2e-3 against the same reference - the recomputed forward augments as the first one did."""
    img, wgt, state, feat_ref, grads_ref = tower_case
    monkeypatch.setenv("MMG_CKPT_KEEP_LAST", keep_last)
    tower = _augmented_tower(dev, state, micro_batch=2, checkpoint=True)
    tower.next_augment_seed = SEED
    feat = tower(img.to(dev))
    tower.next_augment_seed = SEED + 5                   # set between forward and backward: the recomputation must not draw again
    (feat * wgt).sum().backward()
    assert tower.next_augment_seed == SEED + 5
    assert _rel(feat, feat_ref) < 1e-5
    for n, p in tower.model.named_parameters():
        assert _rel(p.grad, grads_ref[n]) < 2e-3, (keep_last, n)


def test_eval_ignores_the_spec_and_raw_pixels_equal_float_pixels(dev, tower_case):
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    img, _, state, _, _ = tower_case
    plain = ConvNextTinyEncoder(micro_batch=4)
    plain.load_state_dict(state)
    plain = plain.to(dev).eval()
    tower = _augmented_tower(dev, state, micro_batch=4).eval()
    as_float = img.to(torch.int32).to(torch.float32) / 65535.0
    with torch.no_grad():
        f_plain_u16, f_plain_f32 = plain(img.to(dev)), plain(as_float.to(dev))
        f_spec = tower(img.to(dev))
        as_u8 = _as_kind(as_float, "uint8")
        f_u8, f_u8_f32 = plain(as_u8.to(dev)), plain((as_u8.to(torch.float32) / 255.0).to(dev))
    assert torch.equal(f_spec, f_plain_u16)               # eval(): no table is passed
    assert torch.equal(f_plain_u16, f_plain_f32)          # uint16 pixels == the same pixels as fp32
    assert torch.equal(f_u8, f_u8_f32)
    tower.train()
    tower.set_augment(None)
    with torch.no_grad():
        assert torch.equal(tower(img.to(dev)), f_plain_u16)           # train() without a spec: none either


def test_checkpointed_forward_holds_less_on_raw_pixels(dev, tower_case, monkeypatch):
    """Between a checkpointed forward and its backward the record holds the pixels: 2 bytes each for uint16, 4 for their fp32 copy
    (torch.cuda.memory_allocated, pixels uploaded inside the measured window, every micro-batch recomputed)."""
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    img, wgt, state, _, _ = tower_case
    monkeypatch.setenv("MMG_CKPT_KEEP_LAST", "0")
    as_float = img.to(torch.int32).to(torch.float32) / 65535.0
    held, feats = {}, {}
    for name, pix in (("uint16", img), ("float32", as_float)):
        tower = ConvNextTinyEncoder(micro_batch=2, checkpoint=True)
        tower.load_state_dict(state)
        tower = tower.to(dev)
        tower(pix[:2].to(dev)).sum().backward()            # materialise arenas / working copies before measuring
        tower.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        feat = tower(pix.to(dev))
        torch.cuda.synchronize()
        held[name] = torch.cuda.memory_allocated() - base
        (feat * wgt).sum().backward()
        torch.cuda.synchronize()
        feats[name] = feat.detach().clone()
        del tower, feat
    print("held by a checkpointed forward:", held)
    assert torch.equal(feats["uint16"], feats["float32"])
    assert held["uint16"] < held["float32"], held
    assert held["float32"] - held["uint16"] >= img.numel(), held          # at least a byte per pixel less (2 in exact arithmetic)


def test_list_of_sizes_rows_are_those_of_each_image_alone(dev):
    """Three uint16 images of two sizes with augmentation, micro_batch = 2: row i == the row of image i run alone under sample_ids=[i] and the
    same seed - a row's parameters depend on (seed, sample id) only, not on the grouping by size."""
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    torch.manual_seed(0)
    tower = ConvNextTinyEncoder(micro_batch=2, augment=EVERY_KNOB._asdict()).to(dev)
    g = torch.Generator().manual_seed(11)
    images = [_as_kind(torch.rand(1, h, w, generator=g), "uint16").to(dev) for h, w in ((64, 48), (40, 72), (64, 48))]
    with torch.no_grad():
        tower.next_augment_seed = SEED
        together = tower(images)
        for i, im in enumerate(images):
            tower.next_augment_seed = SEED
            alone = tower([im], sample_ids=[i])
            assert torch.equal(alone[0], together[i]), i
            tower.next_augment_seed = SEED
            assert torch.equal(tower(im[None], sample_ids=[i])[0], together[i]), i      # and as a 4-D tensor
        tower.next_augment_seed = SEED
        assert not torch.equal(tower([images[1]], sample_ids=[0])[0], together[1])      # another id: another draw
    with pytest.raises(ValueError):
        tower(images, sample_ids=[0, 1])


# ---- 4. the ViT tower ---------------------------------------------------------------------------------------------------------------------
def test_vit_raw_pixels_with_a_flip_equal_the_flipped_float_pixels(dev):
    from mmgclip.networks.vit import ViTTower
    torch.manual_seed(0)
    img = _as_kind(torch.rand(2, 1, 32, 32, generator=torch.Generator().manual_seed(12)), "uint16")
    plain = ViTTower(image_size=32, layers=1)
    state = {k: v.clone() for k, v in plain.state_dict().items()}
    plain = plain.to(dev)
    tower = ViTTower(image_size=32, layers=1, augment=dict(hflip=1.0))
    tower.load_state_dict(state)
    tower = tower.to(dev)
    geom, tone = A.draw(tower.augment, SEED, range(2))
    assert [r[0] for r in geom] == [1, 1]
    pre = R.augmented_images(img, geom, tone)
    assert torch.equal(pre, R.unit_pixels(img).flip(-1))
    tower.next_augment_seed = SEED
    feat = tower(img.to(dev))
    ref = plain(pre.to(dev))
    assert torch.isfinite(feat).all() and torch.equal(feat, ref)
    feat.sum().backward()
    ref.sum().backward()
    for (n, p), (_, q) in zip(tower.model.named_parameters(), plain.model.named_parameters()):
        assert _rel(p.grad, q.grad) < 2e-3, n
    with torch.no_grad():
        assert torch.equal(tower.eval()(img.to(dev)), plain.eval()(R.unit_pixels(img).to(dev)))       # eval(): no flip
        assert torch.equal(tower([t.to(dev) for t in img]), plain(img.to(dev)))                       # a list of same-size images


# ---- 5. the whole model ---------------------------------------------------------------------------------------------------------------------
def _three_losses(tmp, seed):
    """Three steps of train.py's experiment on ConvNeXt-T pixels + (2-layer) BERT: uint16 pixels by dataset.config.pixel_dtype, the example
    augmentation config.  Model and data are the same in every call; `seeding(seed)` decides the augmentation alone."""
    from mmgclip.config import compose
    from mmgclip.dataset.synthetic import SyntheticLoader
    from mmgclip.experiments.experiments_controller import create_experiment
    from mmgclip.networks import bert
    from mmgclip.utils.global_utils import seeding
    cfg = compose(CFG_DIR, "train_binary_class_clf",
                  ["networks=clip_convnexttiny_bert_pixels", "tokenizer=bert_clinical_seqlen=77", "networks/dropout=dropout0",
                   "networks.image_encoder.micro_batch=4", "networks.image_encoder.image_size=64", "scheduler=warmup1_epo15",
                   "+networks/image_encoder/augment=mammo", "dataset.config.pixel_dtype=uint16", "optimizer.config.fused=true",
                   "optimizer.config.learning_rate=5e-4", f"checkpoints.checkpoints_export_dir={tmp}/ckpt", f"base.tensorboard_export_dir={tmp}/tb"])
    loader = SyntheticLoader(1, 8, seed=5, S=77, image_size=64, vocab_size=3000, pixel_dtype=cfg.dataset.config.pixel_dtype)
    assert next(iter(loader))["image"].dtype == torch.uint16
    orig = bert.BertConfigLite.__init__

    def small(self, **kw):
        kw.setdefault("num_hidden_layers", 2)
        kw.setdefault("vocab_size", 3000)
        orig(self, **kw)
    bert.BertConfigLite.__init__ = small
    try:
        torch.manual_seed(0)
        exp = create_experiment("classification")(config=cfg, train_dataloader=loader, valid_dataloader=None, test_dataloader=None,
                                                  tokenizer=None, comm=None)
    finally:
        bert.BertConfigLite.__init__ = orig
    assert exp.model.image_encoder.augment == A.AugmentSpec(0.5, 0.0, 32, (0.9, 1.1), (-0.05, 0.05))
    with torch.no_grad():
        for n, p in exp.model.named_parameters():
            if n.endswith("layer_scale"):
                p.fill_(0.5)
    exp.scheduler.step()                      # leave the reference's lr-0 first epoch
    exp.scheduler.step()
    seeding(seed)
    losses = [float(exp.train()) for _ in range(3)]
    return losses, exp.model.image_encoder._augment_seeds.draw()       # (+ where the augmentation's seed stream stands after three forwards)


def test_whole_model_trains_on_raw_pixels_with_seeded_augmentation(dev, tmp_path):
    """The loss is finite and changes; the same `seeding` gives the same losses, another seed other ones.  "The same" for this model: its
    image tower is bit-reproducible (the tests above), but the contrastive head and the weight gradients sum in fp32 with atomics, whose order
    differs from run to run.  So: the augmentation's seed stream is compared exactly; the first loss - one forward, a mean over 2 x 8
    log-softmax rows in fp32 - to rtol 1e-5 (~100 fp32 roundings); the later losses, which follow weights updated from atomically summed
    gradients, to the rtol 1e-2 that test_fused_adamw_built_before_first_forward_trains_the_towers uses for the same effect.  Another seed must
    leave that band at the first loss already."""
    (a, sa), (b, sb), (c, sc) = (_three_losses(str(tmp_path / t), s) for t, s in (("a", 123), ("b", 123), ("c", 124)))
    print("losses", a, b, c, "next augment seeds", sa, sb, sc)
    assert np.isfinite(a).all() and len(set(a)) == 3, a
    assert sa == sb and sa != sc
    assert np.isclose(a[0], b[0], rtol=1e-5, atol=0) and np.allclose(a, b, rtol=1e-2, atol=0), (a, b)
    assert not np.isclose(a[0], c[0], rtol=1e-2, atol=0), (a, c)
