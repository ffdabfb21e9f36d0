"""Stochastic depth of the ConvNeXt tower, host side (mmgclip/networks/convnext_sd.py): rates, mask, schedule, configuration.  No GPU.

The schedule is a pure function, so it is driven here with a numpy array of sample ids standing in for the activation: the swaps are
applied to that array exactly as mmg_image_swap applies them to the images."""
import os

import numpy as np
import pytest

from mmgclip.networks import convnext_sd as SD
from mmgclip.networks.convnext import CONFIGS, ConvNextTower, group_by_size
from oracle import dropout_oracle as D

CFG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmg-clip_amd", "configs")


@pytest.mark.parametrize("variant,rate", [("tiny", 0.1), ("small", 0.4), ("base", 0.5)])
def test_rates_follow_torchvisions_linear_rule(variant, rate):
    depths = CONFIGS[variant]["depths"]
    B = sum(depths)
    rates = SD.block_rates(rate, depths)
    assert len(rates) == B == {"tiny": 18, "small": 36, "base": 36}[variant]
    b = 0
    for depth in depths:                             # torchvision: sd_prob = p * stage_block_id / (total_stage_blocks - 1.0)
        for _ in range(depth):
            assert rates[b] == rate * b / (B - 1.0)
            b += 1
    assert rates[0] == 0.0 and rates[-1] == rate
    assert SD.scales(rate, depths) == [1.0 / (1.0 - p) for p in rates] and SD.scales(rate, depths)[0] == 1.0


@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("seed", [0, 12345678901234567, 2 ** 62 - 1])
def test_mask_is_the_hash_of_dropout_h(rate, seed):
    rates = SD.block_rates(rate, CONFIGS["tiny"]["depths"])
    ids = np.arange(300)
    keep = SD.keep_matrix(seed, ids, rates)
    assert keep.shape == (18, 300) and keep.dtype == bool
    for b, p in enumerate(rates):
        assert np.array_equal(keep[b], D.keep_mask(ids, p, seed, b)), b
    assert keep[0].all()                             # p_0 = 0: the path without stochastic depth
    assert abs((~keep[-1]).mean() - rate) < 0.1      # (300 draws at p: three sigma is 0.09 at p = 0.5)


def _drive(keep):
    """Execute a schedule on an array of ids; -> (Schedule, kept-prefix / pair / tail assertions made per block)."""
    B, n = keep.shape
    sch = SD.schedule(keep)
    x = np.arange(n)
    history = []
    assert len(sch.steps) == B and sch.n == n
    for b, step in enumerate(sch.steps):
        before = x.copy()
        pairs = sch.table[2 * step.offset: 2 * (step.offset + len(step.pairs))]
        assert tuple(v for pr in step.pairs for v in pr) == tuple(pairs)            # the flattened table holds this block's pairs at its offset
        touched = [v for pr in step.pairs for v in pr]
        assert len(set(touched)) == len(touched)                                    # disjoint
        n_k = step.n_k
        n_d = n - n_k
        assert n_k == int(keep[b].sum()) and len(step.pairs) <= min(n_d, n_k)
        for i, j in step.pairs:
            assert 0 <= i < n_k <= j < n
            x[i], x[j] = x[j], x[i]
        assert set(x[:n_k]) == set(np.flatnonzero(keep[b]))                          # the prefix holds exactly the kept ids
        tail_before = set(before[n_k:]) - set(before[list(touched)])
        assert tail_before <= set(x[n_k:])                                           # untouched tail images stay in the tail ...
        moved = np.flatnonzero(before != x)
        assert set(moved) == set(touched)                                            # ... and nothing but the pairs moves
        history.append(step)
    assert tuple(x) == sch.perm
    return sch, x


@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_schedule_properties(n):
    depths = CONFIGS["tiny"]["depths"]
    seen_none = seen_all = False
    for rate in (0.1, 0.5, 0.95):
        rates = SD.block_rates(rate, depths)
        for seed in range(12):
            keep = SD.keep_matrix(seed * 7919 + 1, np.arange(n), rates)
            sch, x = _drive(keep)
            seen_none |= any(s.n_k == 0 for s in sch.steps)
            seen_all |= any(s.n_k == n for s in sch.steps[1:])      # (block 0 has p = 0 and keeps everything anyway)
            # the final permutation restores input order
            order, inverse = SD.processing_order([list(range(n))], [sch])
            assert order == list(x) and [order[p] for p in inverse] == list(range(n))
            # replaying the swaps backwards is the identity
            for step in reversed(sch.steps):
                for i, j in step.pairs:
                    x[i], x[j] = x[j], x[i]
            assert np.array_equal(x, np.arange(n))
    assert seen_all
    if n <= 7:
        assert seen_none                             # (64 samples all dropped by one block: 0.95^64 = 4 %, not relied on)


def test_both_special_cases_occur_in_the_sweep():
    """n_k = 0 and n_k = n inside one schedule, and a block that needs the full min(n_d, n_k) swaps."""
    rates = SD.block_rates(0.95, CONFIGS["tiny"]["depths"])
    found = False
    for seed in range(50):
        sch = SD.schedule(SD.keep_matrix(seed, np.arange(2), rates))
        ks = [s.n_k for s in sch.steps]
        found |= 0 in ks and 2 in ks and 1 in ks
    assert found
    keep = np.array([[True] * 4, [False, False, True, True], [True, True, False, False], [False] * 4])
    sch = SD.schedule(keep)
    assert [s.n_k for s in sch.steps] == [4, 2, 2, 0]
    assert sch.steps[1].pairs == ((0, 2), (1, 3)) and sch.steps[2].pairs == ((0, 2), (1, 3)) and sch.steps[3].pairs == ()
    assert sch.perm == (0, 1, 2, 3) and sch.table == (0, 2, 1, 3, 0, 2, 1, 3)
    assert [s.offset for s in sch.steps] == [0, 0, 2, 4]


def test_masks_do_not_depend_on_micro_batch_or_grouping():
    rates = SD.block_rates(0.5, CONFIGS["tiny"]["depths"])
    seed, n = 99, 11
    whole = SD.keep_matrix(seed, np.arange(n), rates)
    for mb in (1, 2, 4, 11):                                                         # the tensor path's micro-batches
        got = np.concatenate([SD.keep_matrix(seed, list(range(i, min(i + mb, n))), rates) for i in range(0, n, mb)], 1)
        assert np.array_equal(got, whole)
    sizes = [(64, 64), (96, 64), (64, 64), (32, 32), (96, 64), (64, 64), (64, 64), (32, 32), (96, 64), (64, 64), (64, 64)]
    mbs, inverse = group_by_size(sizes, 2)
    scheds = [SD.schedule(SD.keep_matrix(seed, idx, rates)) for idx in mbs]
    for idx, sch in zip(mbs, scheds):                                                # a sample's column is the one of its input index
        assert np.array_equal(SD.keep_matrix(seed, idx, rates), whole[:, idx])
        assert [s.n_k for s in sch.steps] == list(whole[:, idx].sum(1))
    order, inv = SD.processing_order(mbs, scheds)
    assert sorted(order) == list(range(n)) and [order[p] for p in inv] == list(range(n))
    flat = [i for idx in mbs for i in idx]
    assert all(sorted(order[k:k + len(idx)]) == sorted(idx) for idx, k in zip(mbs, np.cumsum([0] + [len(i) for i in mbs])))
    assert [flat[p] for p in inverse] == list(range(n))                              # (group_by_size's own inverse, for comparison)


def test_constructor_argument_and_range():
    assert ConvNextTower("tiny").stochastic_depth_prob == 0.0
    t = ConvNextTower("tiny", stochastic_depth_prob=0.1)
    assert t.stochastic_depth_prob == 0.1 and t.stochastic_depth_active()
    assert not t.eval().stochastic_depth_active() and not ConvNextTower("tiny").stochastic_depth_active()
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="stochastic_depth_prob"):
            ConvNextTower("tiny", stochastic_depth_prob=bad)
    from mmgclip.networks.encoder import ConvNextBaseEncoder
    assert ConvNextBaseEncoder(stochastic_depth_prob=0.5).stochastic_depth_prob == 0.5


def test_seed_stream_is_private_and_reproducible():
    import torch
    t = ConvNextTower("tiny", stochastic_depth_prob=0.1)
    state = torch.get_rng_state()
    t.reseed_stochastic_depth(7)
    a = [t._drop_seeds.draw() for _ in range(3)]
    t.reseed_stochastic_depth(7)
    assert a == [t._drop_seeds.draw() for _ in range(3)] and len(set(a)) == 3
    t.reseed_stochastic_depth(8)
    assert a[0] != t._drop_seeds.draw()
    assert torch.equal(state, torch.get_rng_state())                                 # torch's global generator is never consumed


def test_config_key_reaches_the_tower(monkeypatch):
    from mmgclip.config import compose
    from mmgclip.networks import bert
    from mmgclip.networks.mmgclip_model import MMGCLIP
    base = ["networks=clip_convnexttiny_bert_pixels", "tokenizer=bert_clinical_seqlen=77"]
    for name in ("clip_convnexttiny_bert_pixels", "clip_convnextbase_bert_pixels"):
        assert compose(CFG_DIR, "train_binary_class_clf", [f"networks={name}"]).networks.image_encoder.stochastic_depth_prob == 0.0
    orig = bert.BertConfigLite.__init__

    def small(self, **kw):                           # (a two-layer text tower: this test is about the image encoder's argument)
        kw.setdefault("num_hidden_layers", 2)
        kw.setdefault("vocab_size", 3000)
        orig(self, **kw)
    monkeypatch.setattr(bert.BertConfigLite, "__init__", small)
    assert MMGCLIP(compose(CFG_DIR, "train_binary_class_clf", base)).image_encoder.stochastic_depth_prob == 0.0
    cfg = compose(CFG_DIR, "train_binary_class_clf", base + ["networks.image_encoder.stochastic_depth_prob=0.1"])
    assert MMGCLIP(cfg).image_encoder.stochastic_depth_prob == 0.1
    for bad in ("1.0", "-0.1"):
        cfg = compose(CFG_DIR, "train_binary_class_clf", base + [f"networks.image_encoder.stochastic_depth_prob={bad}"])
        with pytest.raises(ValueError, match="stochastic_depth_prob"):
            MMGCLIP(cfg)


def test_image_moves_reject_bad_arguments_before_any_hip_call():
    """As everywhere in the library the arguments are validated first, so this runs without a GPU: pair indices out of range, an image
    in two pairs, a width that is no multiple of 8, an image range outside the batch."""
    import ctypes

    from mmgclip import _hip
    lib = _hip.load()
    x, y = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20)        # never dereferenced: every call below is rejected

    def swap(pairs, n=9, rows=49, C=96, dev=x):
        host = (ctypes.c_int * len(pairs))(*pairs)
        return lib.mmg_image_swap(x, dev, host, len(pairs) // 2, n, rows, C, None)
    assert swap([0, 9]) != 0 and b"names image 9 of 9" in lib.mmg_last_error()
    assert swap([-1, 3]) != 0
    assert swap([0, 5, 5, 6]) != 0 and b"two pairs" in lib.mmg_last_error()
    assert swap([2, 2]) != 0
    assert swap([0, 5], C=100) != 0 and b"multiple of 8" in lib.mmg_last_error()
    assert swap([0, 5], dev=None) != 0
    assert lib.mmg_image_swap(ctypes.c_void_p((1 << 20) + 2), x, None, 0, 9, 49, 96, None) != 0 and b"aligned" in lib.mmg_last_error()
    assert lib.mmg_image_swap(x, None, None, 0, 9, 49, 96, None) == 0        # k = 0: nothing to do, no launch
    assert lib.mmg_image_copy(x, y, 7, 3, 9, 49, 96, None) != 0 and b"not inside" in lib.mmg_last_error()
    assert lib.mmg_image_copy(x, y, -1, 1, 9, 49, 96, None) != 0
    assert lib.mmg_image_copy(x, x, 0, 1, 9, 49, 96, None) != 0
    assert lib.mmg_image_copy(x, y, 0, 1, 9, 49, 100, None) != 0 and b"multiple of 8" in lib.mmg_last_error()
    assert lib.mmg_image_copy(x, y, 9, 0, 9, 49, 96, None) == 0              # count = 0: no launch
    assert lib.mmg_scaled_add_f32(x, x, 1.0, 8, None) != 0 and lib.mmg_scaled_add_f32(x, y, 1.0, 0, None) != 0
