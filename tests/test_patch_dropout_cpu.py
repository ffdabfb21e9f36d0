"""Patch dropout of the ViT tower, host side (mmgclip/patch_dropout.py): the draw's structure and statistics, the reference against the
oracle, constructor and configuration, and the library's argument checks.  No GPU.  Every test here fails on the parent commit (no module,
no argument, no symbols)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mmgclip import patch_dropout as PD
from oracle import encoders_oracle as E
from tests import patch_dropout_ref as R

CFG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmg-clip_amd", "configs")
BIG_SEED = 0x1234567890ABCDEF


@pytest.mark.parametrize("P,K", [(36, 18), (36, 1), (36, 36), (289, 216), (4096, 2048)])
def test_rows_are_k_distinct_ascending_indices_and_slot_inverts_them(P, K):
    keep, slot = R.keep_indices(BIG_SEED, [7, 0, 2 ** 31 - 1, 3, 3], P, K)
    assert keep.shape == (5, K) and keep.dtype == np.int32 and slot.shape == (5, P) and slot.dtype == np.int32
    assert keep.min() >= 0 and keep.max() < P
    assert (np.diff(keep, axis=1) > 0).all()                         # ascending, hence distinct
    for b in range(5):
        assert np.array_equal(slot[b, keep[b]], np.arange(K))
        assert (slot[b] >= 0).sum() == K and (slot[b][slot[b] < 0] == -1).all()
    assert np.array_equal(keep[3], keep[4])                          # a row is a function of (seed, sample id) alone


def test_kept_set_is_the_k_smallest_bits_and_bits_never_tie():
    P, K = 289, 100
    bits = PD.patch_bits(BIG_SEED, [0, 5, 2 ** 31 - 1], P)
    assert bits.max() < 2 ** 32
    keep, _ = R.keep_indices(BIG_SEED, [0, 5, 2 ** 31 - 1], P, K)
    for b in range(3):
        assert len(set(bits[b].tolist())) == P                       # mmg_drop_bits is a bijection of p
        kept = np.zeros(P, dtype=bool)
        kept[keep[b]] = True
        assert bits[b][kept].max() < bits[b][~kept].min()
    # the documented formula, in plain Python integers
    from mmgclip.networks.convnext_sd import _fmix32, drop_key
    key = int(_fmix32((drop_key(BIG_SEED, 0x50447270) + 5 * 0xB5297A4D) & 0xFFFFFFFF))
    assert int(bits[1, 17]) == int(_fmix32((17 * 0x9E3779B1 + key) & 0xFFFFFFFF))


def test_hard_cases():
    keep, slot = R.keep_indices(3, [0, 1, 2], 36, 36)                # K = P: the identity
    assert np.array_equal(keep, np.tile(np.arange(36), (3, 1))) and np.array_equal(slot, keep)
    keep, slot = R.keep_indices(3, [0, 1, 2], 36, 1)                 # K = 1
    assert keep.shape == (3, 1) and ((slot >= 0).sum(1) == 1).all()
    for seed in (2 ** 32 + 5, 2 ** 62 - 1, 2 ** 64 - 1):             # seeds above 2^32, a sample id of 2^31 - 1: no overflow
        keep, _ = R.keep_indices(seed, [2 ** 31 - 1, 0], 64, 32)
        assert keep.min() >= 0 and keep.max() < 64
    assert not np.array_equal(R.keep_indices(5, [0], 64, 32)[0], R.keep_indices(2 ** 32 + 5, [0], 64, 32)[0])   # the high word counts
    for bad in (0, 37, -1):
        with pytest.raises(ValueError, match="patch_dropout"):
            R.keep_indices(3, [0], 36, bad)


def test_rows_do_not_depend_on_how_the_input_is_sliced():
    whole = R.keep_indices(11, range(8), 196, 98)
    a, b = R.keep_indices(11, range(4), 196, 98), R.keep_indices(11, range(4, 8), 196, 98)
    assert np.array_equal(whole[0], np.concatenate([a[0], b[0]])) and np.array_equal(whole[1], np.concatenate([a[1], b[1]]))


def test_another_seed_changes_the_set():
    a, b = R.keep_indices(11, range(8), 196, 98)[0], R.keep_indices(12, range(8), 196, 98)[0]
    assert all(not np.array_equal(a[i], b[i]) for i in range(8))


def test_every_patch_is_kept_equally_often():
    """4096 images, P = 36, K = 18: a patch is kept Binomial(4096, 1/2) times, 2048 +- 5 sigma with sigma = 32."""
    keep, _ = R.keep_indices(BIG_SEED, range(4096), 36, 18)
    counts = np.bincount(keep.reshape(-1), minlength=36)
    assert counts.sum() == 4096 * 18
    assert counts.min() >= 1888 and counts.max() <= 2208, (counts.min(), counts.max())
    keep, _ = R.keep_indices(BIG_SEED, range(512), 4096, 2048)       # the C4 shape: 256 +- 5 sigma, sigma = sqrt(512 / 4) = 11.3
    counts = np.bincount(keep.reshape(-1), minlength=4096)
    assert counts.min() >= 200 and counts.max() <= 312, (counts.min(), counts.max())


def test_keep_count_is_open_clips_rule():
    assert [PD.keep_count(36, r) for r in (0.0, 0.25, 0.5, 0.75, 0.99)] == [36, 27, 18, 9, 1]
    assert PD.keep_count(4096, 0.5) == 2048 and PD.keep_count(289, 0.25) == 216 and PD.keep_count(529, 0.5) == 264
    assert PD.keep_count(1, 0.9) == 1
    for P in (36, 196, 4096):
        for r in (0.1, 0.3, 0.7):
            assert PD.keep_count(P, r) == max(1, int(P * (1.0 - r)))


def test_reference_with_the_identity_keep_is_the_oracle():
    from mmgclip.networks.vit import _tv_layout
    torch.manual_seed(0)
    m = _tv_layout(96, 1, 768, 2, 3072, 16)
    with torch.no_grad():
        m.class_token.normal_(std=0.5)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    img = torch.rand(2, 1, 96, 96, generator=torch.Generator().manual_seed(1))
    ident = np.tile(np.arange(36), (2, 1))
    assert torch.equal(R.vit_forward_kept(sd, img, ident), E.vit_forward(sd, img))
    keep, _ = R.keep_indices(4, [0, 1], 36, 18)
    half = R.vit_forward_kept(sd, img, keep)
    assert half.shape == (2, 768) and not torch.equal(half, E.vit_forward(sd, img))
    other = img.clone()                                              # the reference reads no dropped patch
    dropped = sorted(set(range(36)) - set(keep[0].tolist()))[0]
    other[0, :, dropped // 6 * 16:dropped // 6 * 16 + 16, dropped % 6 * 16:dropped % 6 * 16 + 16] = 0.5
    assert torch.equal(R.vit_forward_kept(sd, other, keep), half)


def test_constructor_argument_and_range():
    from mmgclip.networks.encoder import ConvNextTinyEncoder, ResNet50Encoder, ViTB16Encoder
    from mmgclip.networks.vit import ViTTower
    assert ViTTower(image_size=96, layers=1).patch_dropout == 0.0 and not ViTTower(image_size=96, layers=1).patch_dropout_active()
    t = ViTTower(image_size=96, layers=1, patch_dropout=0.5)
    assert t.patch_dropout == 0.5 and t.patch_dropout_active() and t.next_patch_drop_seed is None
    assert not t.eval().patch_dropout_active()
    t.train().patch_dropout = 0.0                                    # reassigned between steps: FLIP's unmasked tuning
    assert not t.patch_dropout_active()
    t.patch_dropout = 0.75
    assert t.patch_dropout == 0.75 and t.patch_dropout_active()
    for bad in (1.0, -0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="patch_dropout"):
            ViTTower(image_size=96, layers=1, patch_dropout=bad)
        with pytest.raises(ValueError, match="patch_dropout"):
            t.patch_dropout = bad
    assert t.patch_dropout == 0.75
    assert ViTB16Encoder(image_size=96, layers=1).patch_dropout == 0.0
    assert ViTB16Encoder(image_size=96, layers=1, patch_dropout=0.5).patch_dropout == 0.5
    for other in (ConvNextTinyEncoder, ResNet50Encoder):             # the key belongs to the ViT tower alone
        with pytest.raises(TypeError, match="patch_dropout"):
            other(patch_dropout=0.5)


def test_seed_stream_is_private_and_reproducible():
    from mmgclip.augment import AugmentSeeds
    from mmgclip.networks.convnext_sd import DropSeeds
    from mmgclip.utils.global_utils import seeding

    def first_draws(cls, base):
        s = cls()
        s.reseed(base)
        return [s.draw() for _ in range(3)]
    state = torch.get_rng_state()
    a = first_draws(PD.PatchDropSeeds, 7)
    assert a == first_draws(PD.PatchDropSeeds, 7) and len(set(a)) == 3 and a != first_draws(PD.PatchDropSeeds, 8)
    assert a != first_draws(DropSeeds, 7) and a != first_draws(AugmentSeeds, 7)      # unrelated to the other streams of the same (seed, rank)
    assert torch.equal(state, torch.get_rng_state())                 # torch's global generator is never consumed
    s = PD.PatchDropSeeds()
    seeding(21)
    b = [s.draw(), s.draw()]
    seeding(21)                                                      # seeding() between two draws restarts the stream
    assert [s.draw(), s.draw()] == b


def test_config_key_reaches_the_tower(monkeypatch):
    from mmgclip.config import compose
    from mmgclip.networks import bert
    from mmgclip.networks.mmgclip_model import MMGCLIP
    base = ["networks=clip_vitb16_bert_pixels", "tokenizer=bert_clinical_seqlen=77", "networks.image_encoder.image_size=96"]
    assert compose(CFG_DIR, "train_binary_class_clf", base[:1]).networks.image_encoder.patch_dropout == 0.0
    orig = bert.BertConfigLite.__init__

    def small(self, **kw):                           # (a two-layer text tower: this test is about the image encoder's argument)
        kw.setdefault("num_hidden_layers", 2)
        kw.setdefault("vocab_size", 3000)
        orig(self, **kw)
    monkeypatch.setattr(bert.BertConfigLite, "__init__", small)
    assert MMGCLIP(compose(CFG_DIR, "train_binary_class_clf", base)).image_encoder.patch_dropout == 0.0
    cfg = compose(CFG_DIR, "train_binary_class_clf", base + ["networks.image_encoder.patch_dropout=0.5"])
    assert MMGCLIP(cfg).image_encoder.patch_dropout == 0.5
    for bad in ("1.0", "-0.1"):
        cfg = compose(CFG_DIR, "train_binary_class_clf", base + [f"networks.image_encoder.patch_dropout={bad}"])
        with pytest.raises(ValueError, match="patch_dropout"):
            MMGCLIP(cfg)


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    """As everywhere in the library the arguments are validated first, so this runs without a GPU."""
    from mmgclip import _hip
    lib = _hip.load()
    a, b, c, d, e = (ctypes.c_void_p(k << 20) for k in range(1, 6))   # never dereferenced: every call below is rejected
    odd = ctypes.c_void_p((1 << 20) + 8)

    def draw(P, K, B=2, keep=a, slot=b):
        return lib.mmg_patch_keep_indices(BIG_SEED, None, B, P, K, keep, slot, None)
    assert draw(16385, 100) != 0 and b"16384" in lib.mmg_last_error()
    assert draw(36, 0) != 0 and b"K=0" in lib.mmg_last_error()
    assert draw(36, 37) != 0 and draw(36, 18, B=0) != 0 and draw(36, 18, keep=None) != 0 and draw(0, 0) != 0

    assert lib.mmg_gather_patch_rows(a, 256, b, c, 2, 36, 37, 256, None) != 0 and b"K=37" in lib.mmg_last_error()
    assert lib.mmg_gather_patch_rows(a, 256, b, c, 2, 36, 18, 252, None) != 0 and b"multiples of 8" in lib.mmg_last_error()
    assert lib.mmg_gather_patch_rows(a, 128, b, c, 2, 36, 18, 256, None) != 0           # ld < Kp
    assert lib.mmg_gather_patch_rows(odd, 256, b, c, 2, 36, 18, 256, None) != 0 and b"aligned" in lib.mmg_last_error()
    assert lib.mmg_gather_patch_rows(a, 256, None, c, 2, 36, 18, 256, None) != 0
    assert lib.mmg_gather_patch_rows(a, 256, b, a, 2, 36, 18, 256, None) != 0            # in place

    assert lib.mmg_vit_assemble_keep_fwd(a, b, c, d, e, 2, 36, 18, 772, None) != 0 and b"H=772" in lib.mmg_last_error()
    assert lib.mmg_vit_assemble_keep_fwd(a, b, c, d, e, 2, 36, 0, 768, None) != 0
    assert lib.mmg_vit_assemble_keep_fwd(a, b, c, None, e, 2, 36, 18, 768, None) != 0
    assert lib.mmg_vit_assemble_keep_fwd(a, odd, c, d, e, 2, 36, 18, 768, None) != 0 and b"aligned" in lib.mmg_last_error()

    assert lib.mmg_vit_assemble_keep_bwd(a, b, c, d, e, 2, 36, 18, 772, None) != 0 and b"H=772" in lib.mmg_last_error()
    assert lib.mmg_vit_assemble_keep_bwd(a, b, c, d, e, 2, 36, 37, 768, None) != 0
    assert lib.mmg_vit_assemble_keep_bwd(a, None, c, d, e, 2, 36, 18, 768, None) != 0
    assert lib.mmg_vit_assemble_keep_bwd(a, b, c, odd, e, 2, 36, 18, 768, None) != 0 and b"aligned" in lib.mmg_last_error()
    assert lib.mmg_abi_version() == 5
