"""The foreground prior of the ViT tower's patch dropout, host side (mmgclip/patch_dropout.py): the numpy draw's structure, the count's
restatement against the torch reference, every validator, the two entry points' argument checks and the constructor.  No GPU.  Every test
here fails on the parent commit (no functions, no symbols, no arguments)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mmgclip import patch_dropout as PD
from tests import patch_prior_ref as PR

CFG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmg-clip_amd", "configs")
BIG_SEED = 0x1234567890ABCDEF
IDS = [7, 0, 2 ** 31 - 1, 3, 3]


def _counts_with(nfg_rows, NP, seed=0):
    """int32 [B, NP]: row b has exactly nfg_rows[b] patches of count 1 (at seeded places), the others 0."""
    rng = np.random.default_rng(seed)
    counts = np.zeros((len(nfg_rows), NP), dtype=np.int32)
    for b, nfg in enumerate(nfg_rows):
        counts[b, rng.permutation(NP)[:nfg]] = 1
    return counts


# ---- the numpy draw -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NP,K", [(36, 18), (289, 100), (1025, 3)])
def test_every_foreground_patch_goes_before_any_background_patch(NP, K):
    nfgs = [0, 1, K - 1, K, K + 1, NP][:5] if NP == 36 else [K - 1, K, K + 1, NP // 2, 1]
    counts = _counts_with(nfgs, NP, seed=NP)
    keep, slot, nfg = PD.keep_indices_prior(BIG_SEED, IDS, counts, 1, K)
    bits = PD.patch_bits(BIG_SEED, IDS, NP)
    assert keep.shape == (5, K) and keep.dtype == np.int32 and slot.shape == (5, NP) and slot.dtype == np.int32
    assert nfg.dtype == np.int32 and nfg.tolist() == nfgs
    assert (np.diff(keep, axis=1) > 0).all() and keep.min() >= 0 and keep.max() < NP
    for b in range(5):
        fg = counts[b] >= 1
        kept = np.zeros(NP, dtype=bool)
        kept[keep[b]] = True
        assert np.array_equal(slot[b, keep[b]], np.arange(K)) and (slot[b][~kept] == -1).all()
        assert (kept & fg).sum() == min(K, nfgs[b])                  # as much tissue as K holds
        if nfgs[b] >= K:                                             # a K-subset of the foreground: the smallest bits among it
            assert not (kept & ~fg).any()
            if nfgs[b] > K:
                assert bits[b][kept].max() < bits[b][fg & ~kept].min()
        else:                                                        # all foreground, then the background patches of smallest bits
            assert (kept | ~fg).all()
            if K - nfgs[b] < NP - nfgs[b] and K > nfgs[b]:
                assert bits[b][kept & ~fg].max() < bits[b][~fg & ~kept].min()
        # the statement itself: the K smallest (class, bits) keys
        key = bits[b].astype(object) + (~fg).astype(object) * 2 ** 32
        assert sorted(keep[b].tolist()) == sorted(np.argsort(key, kind="stable")[:K].tolist())


@pytest.mark.parametrize("NP,K", [(36, 18), (1024, 512), (4097, 4000)])
def test_rows_of_one_class_equal_the_uniform_draw(NP, K):
    ref_keep, ref_slot = PD.keep_indices(BIG_SEED, IDS, NP, K)
    for fill, want in ((0, 0), (5, NP)):
        keep, slot, nfg = PD.keep_indices_prior(BIG_SEED, IDS, np.full((5, NP), fill, dtype=np.int32), 1, K)
        assert np.array_equal(keep, ref_keep) and np.array_equal(slot, ref_slot) and nfg.tolist() == [want] * 5
    mixed = np.zeros((5, NP), dtype=np.int32)                        # rows 1 and 3 mixed: only they may differ
    mixed[1, :NP // 2] = mixed[3, 1::2] = 1
    mixed[4] = 1
    keep, slot, nfg = PD.keep_indices_prior(BIG_SEED, IDS, mixed, 1, K)
    for b in (0, 2, 4):
        assert np.array_equal(keep[b], ref_keep[b]) and np.array_equal(slot[b], ref_slot[b])
    if K < NP:
        assert not np.array_equal(keep[1], ref_keep[1])


def test_k_around_the_foreground_boundary():
    NP, nfg = 64, 20
    counts = _counts_with([nfg] * 3, NP, seed=1)
    for K in (nfg - 1, nfg, nfg + 1):
        keep, _, n = PD.keep_indices_prior(5, [0, 1, 2], counts, 1, K)
        assert n.tolist() == [nfg] * 3
        for b in range(3):
            fg_kept = int((counts[b, keep[b]] >= 1).sum())
            assert fg_kept == min(K, nfg) and K - fg_kept == max(0, K - nfg)
    keep_at, _, _ = PD.keep_indices_prior(5, [0, 1, 2], counts, 1, nfg)      # K = nfg: exactly the foreground
    for b in range(3):
        assert np.array_equal(keep_at[b], np.flatnonzero(counts[b] >= 1))
    keep_lo, _, _ = PD.keep_indices_prior(5, [0, 1, 2], counts, 1, nfg - 1)   # nested: K - 1 drops one patch of K's set
    keep_hi, _, _ = PD.keep_indices_prior(5, [0, 1, 2], counts, 1, nfg + 1)
    for b in range(3):
        assert set(keep_lo[b]) < set(keep_at[b]) < set(keep_hi[b])


def test_min_pixels_is_the_class_boundary():
    counts = np.tile(np.arange(5, dtype=np.int32), (2, 4))           # counts 0..4, four times: NP = 20
    keep1, _, n1 = PD.keep_indices_prior(9, [0, 1], counts, 1, 16)   # min_pixels 1: counts 1..4 are foreground, 16 patches
    assert n1.tolist() == [16, 16]
    for b in range(2):
        assert np.array_equal(keep1[b], np.flatnonzero(counts[b] >= 1))
    keep3, _, n3 = PD.keep_indices_prior(9, [0, 1], counts, 3, 8)    # min_pixels 3: counts 3, 4 are, 8 patches
    assert n3.tolist() == [8, 8]
    for b in range(2):
        assert np.array_equal(keep3[b], np.flatnonzero(counts[b] >= 3))
    for bad in (0, -1):
        with pytest.raises(ValueError, match="patch_min_pixels"):
            PD.keep_indices_prior(9, [0, 1], counts, bad, 8)
    for bad in (0, 21):
        with pytest.raises(ValueError, match="patch_dropout"):
            PD.keep_indices_prior(9, [0, 1], counts, 1, bad)


def test_rows_do_not_depend_on_how_the_input_is_sliced():
    counts = _counts_with([10, 50, 98, 99, 150, 196, 0, 3], 196, seed=2)
    whole = PD.keep_indices_prior(11, range(8), counts, 1, 98)
    a, b = PD.keep_indices_prior(11, range(4), counts[:4], 1, 98), PD.keep_indices_prior(11, range(4, 8), counts[4:], 1, 98)
    for k in range(3):
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]]))


# ---- the count ------------------------------------------------------------------------------------------------------------------------------
def test_numpy_count_equals_the_torch_reference_and_pins_greater_than():
    t = 0.25
    up = float(np.nextafter(np.float32(t), np.float32(1)))
    g = torch.Generator().manual_seed(3)
    img = torch.tensor([0.0, t, up])[torch.randint(0, 3, (2, 3, 70, 50), generator=g)]
    img[0, 0, 3, 5] = float("nan")
    ref = PR.foreground_counts(img, 16, t)
    assert ref.shape == (2, 4 * 3) and ref.dtype == torch.int32
    assert np.array_equal(PD.foreground_counts(img.numpy(), 16, t), ref.numpy())
    exact = (img[:, :, :64, :48] == up).reshape(2, 3, 4, 16, 3, 16).sum(dim=(1, 3, 5)).reshape(2, 12)
    assert torch.equal(ref, exact.to(torch.int32))                   # t itself and NaN are background
    geom = [[1, 0, 0, 0], [2, -5, 7, 0]]
    assert np.array_equal(PD.foreground_counts(PR.canvas01(img, geom).numpy(), 16, t), PR.foreground_counts(img, 16, t, geom).numpy())
    u16 = torch.randint(0, 65536, (1, 1, 32, 32), generator=g).to(torch.int32).to(torch.uint16)
    want = (u16.to(torch.int32).to(torch.float32) / 65535.0 > 0.5).reshape(1, 2, 16, 2, 16).sum(dim=(2, 4)).reshape(1, 4)
    assert torch.equal(PR.foreground_counts(u16, 16, 0.5), want.to(torch.int32))


# ---- validators ---------------------------------------------------------------------------------------------------------------------------
def test_validators_accept_and_reject():
    assert [PD.check_prior(p) for p in ("uniform", "foreground")] == ["uniform", "foreground"]
    for bad in ("Foreground", "", None, 0, True, b"uniform"):
        with pytest.raises(ValueError, match="patch_prior"):
            PD.check_prior(bad)
    assert PD.check_threshold(0) == 0.0 and PD.check_threshold(0.25) == 0.25 and PD.check_threshold(np.float32(0.5)) == 0.5
    assert PD.check_threshold(float(np.nextafter(1.0, 0.0))) < 1.0
    for bad in (1.0, 1, -0.1, 1.5, float("nan"), float("inf"), -float("inf"), "0.5", None, True, False):
        with pytest.raises(ValueError, match="patch_threshold"):
            PD.check_threshold(bad)
    assert PD.check_min_pixels(1, 256) == 1 and PD.check_min_pixels(256, 256) == 256 and PD.check_min_pixels(np.int64(3), 768) == 3
    for bad in (0, -1, 257, 1.0, 2.5, "3", None, True, False, float("nan")):
        with pytest.raises(ValueError, match="patch_min_pixels"):
            PD.check_min_pixels(bad, 256)
    assert PD.check_dropout_eval(False, "uniform") is False and PD.check_dropout_eval(False, "foreground") is False
    assert PD.check_dropout_eval(True, "foreground") is True
    with pytest.raises(ValueError, match="patch_dropout_eval"):
        PD.check_dropout_eval(True, "uniform")
    for bad in (1, 0, "true", None, 1.0):
        with pytest.raises(ValueError, match="patch_dropout_eval"):
            PD.check_dropout_eval(bad, "foreground")


# ---- the library's argument checks --------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_before_any_hip_call():
    """As everywhere in the library the arguments are validated first, so this runs without a GPU."""
    from mmgclip import _hip
    lib = _hip.load()
    a, b, c, d, e = (ctypes.c_void_p(k << 20) for k in range(1, 6))   # never dereferenced: every call below is rejected
    odd = ctypes.c_void_p((1 << 20) + 1)

    def count(img=a, kind=0, n=2, Cin=1, H=64, W=64, patch=16, geom=None, thr=0.25, counts=b):
        return lib.mmg_patch_foreground(img, kind, n, Cin, H, W, patch, geom, thr, counts, None)
    assert count(img=None) != 0 and b"null img" in lib.mmg_last_error()
    assert count(counts=None) != 0 and b"null counts" in lib.mmg_last_error()
    assert count(kind=3) != 0 and b"src_kind 3" in lib.mmg_last_error()
    assert count(kind=-1) != 0
    assert count(patch=0) != 0 and b"patch=0" in lib.mmg_last_error()
    assert count(patch=-16) != 0 and count(n=0) != 0 and count(Cin=0) != 0 and count(H=8) != 0 and count(W=15) != 0
    assert count(thr=1.0) != 0 and b"threshold" in lib.mmg_last_error()
    assert count(thr=-0.5) != 0 and count(thr=float("nan")) != 0
    assert count(img=odd, kind=1) != 0 and b"misaligned" in lib.mmg_last_error()
    assert count(geom=odd) != 0 and b"misaligned" in lib.mmg_last_error()

    def draw(NP, K, B=2, counts=c, min_pixels=1, keep=a, slot=b, nfg=d):
        return lib.mmg_patch_keep_indices_prior(BIG_SEED, None, counts, min_pixels, B, NP, K, keep, slot, nfg, None)
    assert draw(16385, 100) != 0 and b"16384" in lib.mmg_last_error()
    assert draw(36, 0) != 0 and b"K=0" in lib.mmg_last_error()
    assert draw(36, 37) != 0 and b"K=37" in lib.mmg_last_error()
    assert draw(36, 18, min_pixels=0) != 0 and b"min_pixels=0" in lib.mmg_last_error()
    assert draw(36, 18, min_pixels=-3) != 0
    assert draw(36, 18, counts=None) != 0 and draw(36, 18, keep=None) != 0 and draw(36, 18, slot=None) != 0
    assert draw(36, 18, B=0) != 0 and draw(0, 0) != 0
    assert lib.mmg_abi_version() == 5


# ---- constructor and configuration --------------------------------------------------------------------------------------------------------
def test_constructor_arguments_and_ranges():
    from mmgclip.networks.encoder import ConvNextTinyEncoder, ViTB16Encoder
    from mmgclip.networks.vit import ViTTower
    t = ViTTower(image_size=96, layers=1)
    assert (t.patch_prior, t.patch_threshold, t.patch_min_pixels, t.patch_dropout_eval) == ("uniform", 0.0, 1, False)
    assert t.last_patch_foreground is None
    t = ViTTower(image_size=96, layers=1, patch_dropout=0.5, patch_prior="foreground", patch_threshold=0.05, patch_min_pixels=8,
                 patch_dropout_eval=True)
    assert (t.patch_prior, t.patch_threshold, t.patch_min_pixels, t.patch_dropout_eval) == ("foreground", 0.05, 8, True)
    assert t.patch_dropout_active() and t.eval().patch_dropout_active()          # the switch keeps K patches under eval() too
    t.patch_dropout_eval = False
    assert not t.patch_dropout_active() and t.train().patch_dropout_active()
    t.patch_prior = "uniform"                                        # reassigned between steps, like patch_dropout
    t.patch_threshold, t.patch_min_pixels = 0.5, 256
    assert (t.patch_prior, t.patch_threshold, t.patch_min_pixels) == ("uniform", 0.5, 256)
    with pytest.raises(ValueError, match="patch_dropout_eval"):
        t.patch_dropout_eval = True                                  # needs the foreground prior
    t.patch_prior = "foreground"
    t.patch_dropout_eval = True
    with pytest.raises(ValueError, match="patch_dropout_eval"):
        t.patch_prior = "uniform"                                    # ... and keeps needing it
    assert t.patch_prior == "foreground" and t.patch_dropout_eval is True
    for kw, match in (({"patch_prior": "tissue"}, "patch_prior"), ({"patch_prior": None}, "patch_prior"),
                      ({"patch_threshold": 1.0}, "patch_threshold"), ({"patch_threshold": float("nan")}, "patch_threshold"),
                      ({"patch_threshold": True}, "patch_threshold"), ({"patch_threshold": -0.01}, "patch_threshold"),
                      ({"patch_min_pixels": 0}, "patch_min_pixels"), ({"patch_min_pixels": 257}, "patch_min_pixels"),
                      ({"patch_min_pixels": True}, "patch_min_pixels"), ({"patch_min_pixels": 2.0}, "patch_min_pixels"),
                      ({"patch_dropout_eval": True}, "patch_dropout_eval"),
                      ({"patch_dropout_eval": True, "patch_prior": "uniform"}, "patch_dropout_eval"),
                      ({"patch_dropout_eval": 1, "patch_prior": "foreground"}, "patch_dropout_eval")):
        with pytest.raises(ValueError, match=match):
            ViTTower(image_size=96, layers=1, **kw)
    assert ViTTower(image_size=96, layers=1, in_chans=3, patch_min_pixels=768).patch_min_pixels == 768      # Cin * patch^2
    e = ViTB16Encoder(image_size=96, layers=1, patch_dropout=0.5, patch_prior="foreground", patch_threshold=0.1, patch_min_pixels=4,
                      patch_dropout_eval=True)
    assert (e.patch_prior, e.patch_threshold, e.patch_min_pixels, e.patch_dropout_eval) == ("foreground", 0.1, 4, True)
    assert ViTB16Encoder(image_size=96, layers=1).patch_prior == "uniform"
    with pytest.raises(TypeError, match="patch_prior"):
        ConvNextTinyEncoder(patch_prior="foreground")                # the keys belong to the ViT tower alone


def test_config_keys_reach_the_tower(monkeypatch):
    from mmgclip.config import compose
    from mmgclip.networks import bert
    from mmgclip.networks.mmgclip_model import MMGCLIP
    base = ["networks=clip_vitb16_bert_pixels", "tokenizer=bert_clinical_seqlen=77", "networks.image_encoder.image_size=96"]
    orig = bert.BertConfigLite.__init__

    def small(self, **kw):                           # (a two-layer text tower: this test is about the image encoder's arguments)
        kw.setdefault("num_hidden_layers", 2)
        kw.setdefault("vocab_size", 3000)
        orig(self, **kw)
    monkeypatch.setattr(bert.BertConfigLite, "__init__", small)
    enc = MMGCLIP(compose(CFG_DIR, "train_binary_class_clf", base)).image_encoder            # the shipped config: the defaults
    assert (enc.patch_prior, enc.patch_threshold, enc.patch_min_pixels, enc.patch_dropout_eval) == ("uniform", 0.0, 1, False)
    ie = "networks.image_encoder."
    cfg = compose(CFG_DIR, "train_binary_class_clf", base + [ie + "patch_dropout=0.5", ie + "patch_prior=foreground", ie + "patch_threshold=0.02",
                                                             ie + "patch_min_pixels=16", ie + "patch_dropout_eval=true"])
    enc = MMGCLIP(cfg).image_encoder
    assert (enc.patch_dropout, enc.patch_prior, enc.patch_threshold, enc.patch_min_pixels, enc.patch_dropout_eval) == \
        (0.5, "foreground", 0.02, 16, True)
    for bad, match in ((ie + "patch_prior=centre", "patch_prior"), (ie + "patch_threshold=1.0", "patch_threshold"),
                       (ie + "patch_min_pixels=0", "patch_min_pixels"), (ie + "patch_dropout_eval=true", "patch_dropout_eval")):
        with pytest.raises(ValueError, match=match):
            MMGCLIP(compose(CFG_DIR, "train_binary_class_clf", base + [bad]))
