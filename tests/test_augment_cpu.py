"""mmgclip/augment.py (the draw, plain Python), tests/augment_ref.py (the CPU reference of mmg_patchify_aug) and the new entry's argument
checks - all without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mmgclip import augment as A
from tests import augment_ref as R

FULL = A.AugmentSpec(hflip=0.5, vflip=0.25, max_shift=32, gain=(0.9, 1.1), offset=(-0.05, 0.05))
SEED = 20240611


def test_draw_is_deterministic_and_a_function_of_seed_and_sample_id():
    ids = list(range(64))
    geom, tone = A.draw(FULL, SEED, ids)
    assert (geom, tone) == A.draw(FULL, SEED, ids)
    assert all(len(r) == 4 and r[3] == 0 and all(isinstance(v, int) for v in r) for r in geom) and all(len(r) == 2 for r in tone)
    perm = np.random.default_rng(0).permutation(64).tolist()
    gp, tp = A.draw(FULL, SEED, perm)
    assert gp == [geom[i] for i in perm] and tp == [tone[i] for i in perm]
    sub = [5, 63, 17]
    gs, ts = A.draw(FULL, SEED, sub)
    assert gs == [geom[i] for i in sub] and ts == [tone[i] for i in sub]
    # a dict (a config node) is the same spec
    assert A.draw(dict(FULL._asdict()), SEED, ids) == (geom, tone)


def test_different_seeds_and_ranks_give_different_tables(monkeypatch):
    ids = list(range(32))
    assert A.draw(FULL, SEED, ids) != A.draw(FULL, SEED + 1, ids)
    from mmgclip.utils.global_utils import seeding
    from mmgclip.networks.convnext_sd import DropSeeds

    def first_draws(rank, base, cls=A.AugmentSeeds):
        monkeypatch.setenv("RANK", str(rank))
        seeding(base)
        s = cls()
        return [s.draw() for _ in range(3)]
    a, b = first_draws(0, 7), first_draws(1, 7)
    assert a == first_draws(0, 7)                       # seeding(s) reproduces the stream
    assert a != b and a != first_draws(0, 8)            # another rank, another base seed
    assert a != first_draws(0, 7, DropSeeds)            # unrelated to the stochastic-depth stream of the same (seed, rank)
    assert A.draw(FULL, a[0], ids) != A.draw(FULL, b[0], ids)
    s = A.AugmentSeeds()                                # seeding() between two draws restarts the stream
    seeding(7)
    x = s.draw()
    seeding(7)
    assert s.draw() == x


def test_flip_share_shift_range_and_tone_ranges():
    ids = list(range(4096))
    geom, tone = A.draw(FULL, SEED, ids)
    share = sum(r[0] & 1 for r in geom) / 4096.0
    assert 0.461 <= share <= 0.539, share                 # 5 binomial sigma at p = 0.5, n = 4096; the hash is deterministic
    vshare = sum((r[0] >> 1) & 1 for r in geom) / 4096.0
    assert abs(vshare - 0.25) <= 5 * (0.25 * 0.75 / 4096) ** 0.5, vshare
    assert all(r[0] in (0, 1, 2, 3) for r in geom)
    for col in (1, 2):
        vals = [r[col] for r in geom]
        assert min(vals) == -32 and max(vals) == 32, (col, min(vals), max(vals))      # inside, and both ends reached (4096 draws of 65 values)
    assert [r[1] for r in geom] != [r[2] for r in geom]    # ty and tx draw under sites of their own
    assert all(0.9 <= g <= 1.1 and -0.05 <= o <= 0.05 for g, o in tone)
    gains, offs = np.array([t[0] for t in tone]), np.array([t[1] for t in tone])
    assert gains.min() < 0.91 and gains.max() > 1.09 and offs.min() < -0.045 and offs.max() > 0.045
    assert A.draw(A.AugmentSpec(hflip=1.0, vflip=1.0), SEED, ids)[0] == [[3, 0, 0, 0]] * 4096


def test_identity_spec_draws_identity_rows():
    for spec in (A.AugmentSpec(), dict(hflip=0.0, vflip=0.0, max_shift=0, gain=[1, 1], offset=[0, 0]), {}):
        geom, tone = A.draw(spec, SEED, range(257))
        assert geom == [[0, 0, 0, 0]] * 257 and tone == [[1.0, 0.0]] * 257
    assert A.make_spec(None) is None


@pytest.mark.parametrize("bad", [dict(hflip=-0.1), dict(hflip=1.5), dict(vflip=float("nan")), dict(max_shift=-1), dict(max_shift=2.5),
                                 dict(gain=[0.0, 1.0]), dict(gain=[1.2, 1.1]), dict(gain=[-1.0, 1.0]), dict(gain=1.0), dict(gain=[1.0]),
                                 dict(offset=[0.1, -0.1]), dict(offset=[0.0, float("inf")]), dict(rotate=5), dict(hflip="often"),
                                 dict(hflip=True), 0.5, [0.5]])
def test_bad_specs_raise(bad):
    with pytest.raises(ValueError):
        A.make_spec(bad)


@pytest.mark.parametrize("cin,kp", [(1, 32), (3, 64)])
def test_reference_with_identity_parameters_is_the_unfold_formula(cin, kp):
    """tests/test_kernels_gpu.py::test_patchify_matches_conv_unfold's formula, here bit for bit (both sides torch fp32 on the CPU), with NULL
    tables and with identity rows."""
    img = torch.rand(2, cin, 32, 48, generator=torch.Generator().manual_seed(14))
    scaled = (img * 65535.0 - 32767.5) / 32767.5
    ref = scaled.reshape(2, cin, 8, 4, 12, 4).permute(0, 2, 4, 3, 5, 1).reshape(2 * 8 * 12, 16 * cin).to(torch.bfloat16)
    for geom, tone in ((None, None), ([[0, 0, 0, 0]] * 2, [[1.0, 0.0]] * 2)):
        p = R.patch_rows(img, 4, kp, True, geom, tone)
        assert torch.equal(p[:, :16 * cin], ref) and (p[:, 16 * cin:] == 0).all()


@pytest.mark.parametrize("scale16", [True, False])
def test_reference_on_all_65536_values_equals_itself_on_the_fp32_pixels(scale16):
    """Integer input == the same values as v / 65535 in fp32, for every 16-bit value, in fp32 before the bf16 rounding and after it; and the
    kernel's one-division form (v - 32767.5) / 32767.5 is the same fp32 number as the two-division definition."""
    v = torch.arange(65536, dtype=torch.int32).to(torch.uint16).reshape(1, 1, 256, 256)
    as_float = v.to(torch.int32).to(torch.float32) / 65535.0
    assert torch.equal(R.scale(R.augmented_images(v), scale16), R.scale(R.augmented_images(as_float), scale16))
    assert torch.equal(R.patch_rows(v, 4, 32, scale16), R.patch_rows(as_float, 4, 32, scale16))
    if scale16:
        short = (v.to(torch.int32).to(torch.float32) - 32767.5) / 32767.5
        assert torch.equal(short, R.scale(R.augmented_images(v), True))
    v8 = torch.arange(256, dtype=torch.int32).to(torch.uint8).reshape(1, 1, 16, 16)
    assert torch.equal(R.patch_rows(v8, 4, 32, scale16), R.patch_rows(v8.to(torch.float32) / 255.0, 4, 32, scale16))


def test_reference_geometry_on_a_hand_checked_image():
    """flip over the FULL width, then shift, then fill: 1 x 1 x 2 x 5 image, flip x and tx = 1."""
    img = torch.tensor([[[[10, 11, 12, 13, 14], [20, 21, 22, 23, 24]]]], dtype=torch.uint8)
    out = R.gather(img, [[1, 0, 1, 0]])
    assert out.tolist() == [[[[0, 14, 13, 12, 11], [0, 24, 23, 22, 21]]]]
    out = R.gather(img, [[2, -1, 0, 0]])                  # flip y, then up by one: canvas row 0 reads flipped row 1 = source row 0
    assert out.tolist() == [[[[10, 11, 12, 13, 14], [0, 0, 0, 0, 0]]]]
    x01 = R.augmented_images(img, [[0, 0, 5, 0]], [[2.0, 0.25]])      # everything fill: tone acts on the fill too
    assert torch.equal(x01, torch.full((1, 1, 2, 5), 0.25))


def test_synthetic_batch_pixel_dtypes_hold_the_same_draws():
    from mmgclip.dataset.synthetic import synthetic_batch
    f = synthetic_batch(3, image_size=(8, 12), seed=9)["image"]
    u16 = synthetic_batch(3, image_size=(8, 12), seed=9, pixel_dtype="uint16")["image"]
    u8 = synthetic_batch(3, image_size=(8, 12), seed=9, pixel_dtype="uint8")["image"]
    assert f.dtype == torch.float32 and u16.dtype == torch.uint16 and u8.dtype == torch.uint8
    assert torch.equal(u16.to(torch.int32), (f * 65535).round().to(torch.int32)) and torch.equal(u8.to(torch.int32), (f * 255).round().to(torch.int32))
    st = synthetic_batch(2, seed=9, views_per_study=(1, 2), view_sizes=[(8, 8)], pixel_dtype="uint16")["image"]
    assert all(v.dtype == torch.uint16 for s in st for v in s)
    with pytest.raises(ValueError):
        synthetic_batch(1, image_size=8, pixel_dtype="int16")


def test_example_config_composes_to_a_valid_spec():
    from mmgclip.config import compose
    cfg_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmg-clip_amd", "configs")
    base = ["networks=clip_convnexttiny_bert_pixels"]
    assert "augment" not in compose(cfg_dir, "train_binary_class_clf", base).networks.image_encoder
    cfg = compose(cfg_dir, "train_binary_class_clf", base + ["+networks/image_encoder/augment=mammo", "dataset.config.pixel_dtype=uint16"])
    assert A.make_spec(cfg.networks.image_encoder.augment) == A.AugmentSpec(0.5, 0.0, 32, (0.9, 1.1), (-0.05, 0.05))
    assert cfg.dataset.config.pixel_dtype == "uint16" and cfg.networks.image_encoder.name == "ConvNextTinyEncoder"


def test_train_loaders_follow_dataset_config_pixel_dtype():
    import train
    from mmgclip.config import compose
    cfg_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmg-clip_amd", "configs")
    over = ["networks=clip_convnexttiny_bert_pixels", "networks.image_encoder.image_size=32", "dataloader.train.batch_size=2",
            "dataloader.valid.batch_size=2", "dataloader.test.batch_size=2"]
    for extra, dtype in (([], torch.float32), (["dataset.config.pixel_dtype=uint16"], torch.uint16), (["dataset.config.pixel_dtype=uint8"], torch.uint8)):
        loaders = train.build_loaders(compose(cfg_dir, "train_binary_class_clf", over + extra))
        for loader in loaders:
            img = next(iter(loader))["image"]
            assert img.dtype == dtype and tuple(img.shape) == (2, 1, 32, 32)


def test_load_image_raw_returns_the_integers(tmp_path):
    from PIL import Image
    from mmgclip.networks.image_features import load_image
    a16 = (np.arange(48, dtype=np.uint32).reshape(6, 8) * 1365).astype(np.uint16)
    a8 = (np.arange(48, dtype=np.uint32).reshape(6, 8) * 5).astype(np.uint8)
    Image.fromarray(a16).save(tmp_path / "m16.png")
    Image.fromarray(a8).save(tmp_path / "m8.png")
    r16, r8 = load_image(str(tmp_path / "m16.png"), raw=True), load_image(str(tmp_path / "m8.png"), raw=True)
    assert r16.dtype == torch.uint16 and r8.dtype == torch.uint8 and tuple(r16.shape) == (1, 6, 8)
    assert np.array_equal(r16[0].numpy(), a16) and np.array_equal(r8[0].numpy(), a8)
    f16, f8 = load_image(str(tmp_path / "m16.png")), load_image(str(tmp_path / "m8.png"))           # the default is unchanged
    assert f16.dtype == torch.float32 and torch.equal(f16, R.unit_pixels(r16)) and torch.equal(f8, R.unit_pixels(r8))


def test_patchify_aug_rejects_bad_arguments_before_any_gpu_call():
    """The new entry exists and checks its arguments on the host: unknown src_kind, null img / out, the shapes mmg_patchify rejects -
    non-zero return and a message, no device needed.  (Fails on the parent commit: the symbol does not exist there.)"""
    from mmgclip import _hip
    lib = _hip.load()
    p = ctypes.c_void_p(4096)

    def rc(*args):
        return lib.mmg_patchify_aug(*args, None, None, None)
    assert rc(p, 7, p, 1, 1, 32, 32, 4, 32, 1) != 0 and "src_kind" in _hip.last_error()
    assert rc(p, -1, p, 1, 1, 32, 32, 4, 32, 1) != 0 and "src_kind" in _hip.last_error()
    assert rc(None, 1, p, 1, 1, 32, 32, 4, 32, 1) != 0 and "null img" in _hip.last_error()
    assert rc(p, 1, None, 1, 1, 32, 32, 4, 32, 1) != 0 and "null out" in _hip.last_error()
    for n, cin, H, W, P, Kp in [(0, 1, 32, 32, 4, 32), (1, 0, 32, 32, 4, 32), (1, 1, 3, 32, 4, 32), (1, 1, 32, 3, 4, 32), (1, 1, 32, 32, 0, 32),
                                (1, 3, 32, 32, 4, 32), (1, 1, 32, 32, 4, 36)]:
        assert rc(p, 1, p, n, cin, H, W, P, Kp, 1) != 0 and "bad argument" in _hip.last_error(), (n, cin, H, W, P, Kp)
    assert lib.mmg_abi_version() == 5
