"""The zero-shot AUROC kernels on the MI355X: csrc/auroc_head.hip through `_hip.call` on the test's own buffers, then `ZeroShotAUROC`
and `ClassifierExperiment.validate()`, against the int64 reference of tests/auroc_ref.py.  Every comparison is exact.

Every kernel call writes into buffers pre-filled with a poison value and followed by sentinel entries; no output may keep its fill and
no sentinel may change.  Weight rows are `ld` = the width padded to 16 plus 16 wide: zeros in the padding to 16 (the contract), 77 in
the 16 columns beyond it, which nothing may count."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import auroc_ref as A

pytestmark = pytest.mark.gpu
TAIL = 32
SENTINEL = 12345
POISON = -77777
SEED = 5


def _rows(w, dev):
    """int [B, m] -> device int8 [B, ceil16(m) + 16]: zeros up to the multiple of 16, 77 beyond."""
    w = np.asarray(w)
    B, m = w.shape
    out = torch.full((B, (m + 15) // 16 * 16 + 16), 77, dtype=torch.int8)
    out[:, :(m + 15) // 16 * 16] = 0
    out[:, :m] = torch.from_numpy(w.astype(np.int8))
    return out.to(dev).contiguous()


def _pairs(dev, s_pos, s_neg, w_pos, w_neg, rows=None):
    """One launch on a fresh, poisoned partial buffer -> U2 int64 [B] (CPU).  `rows` = (a, b): the positives a..b-1 only, handed
    over as offset pointers into the same buffers."""
    from mmgclip._hip import call, ptr, stream
    a, b = rows if rows is not None else (0, len(s_pos))
    sp, sn = torch.from_numpy(np.asarray(s_pos, dtype=np.float32)).to(dev), torch.from_numpy(np.asarray(s_neg, dtype=np.float32)).to(dev)
    wp, wn = _rows(w_pos, dev), _rows(w_neg, dev)
    P, Nn, B = b - a, len(s_neg), wn.shape[0]
    blocks = (P + 31) // 32
    partial = torch.full((blocks * B + TAIL,), SENTINEL, device=dev, dtype=torch.int64)
    partial[:blocks * B] = POISON
    call("mmg_auroc_pairs", ctypes.c_void_p(sp.data_ptr() + 4 * a), ptr(sn), ctypes.c_void_p(wp.data_ptr() + a), wp.shape[1], ptr(wn),
         wn.shape[1], P, Nn, B, ptr(partial), stream())
    torch.cuda.synchronize()
    assert bool((partial[blocks * B:] == SENTINEL).all()), "a sentinel after the output changed"
    out = partial[:blocks * B].cpu().view(blocks, B)
    assert not bool((out == POISON).any()), "an owned element kept its fill"
    return out.sum(dim=0)


def _scores(kind, n, seed):
    if kind == "ties":
        return A.tie_scores(n, seed)
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def test_one_hot_weights_pin_the_operand_maps(dev):
    """P = Nn = B = 96, w+ one-hot at (b, i_b) and w- one-hot at (b, j_b): U2[b] = g(s+_{i_b}, s-_{j_b}).  Over the launches every
    replicate, every positive and every negative of the middle 32 x 32 x 32 block is hit, with the first and last positions of the
    blocks around it; the affine maps differ, so a replicate never meets the same pair twice."""
    n = 96
    s_pos, s_neg = _scores("ties", n, 1), _scores("ties", n, 2)
    G = A.g_matrix(s_pos, s_neg)
    assert sorted(np.unique(G).tolist()) == [0, 1, 2]
    seen_i, seen_j = set(), set()
    for mul_i, add_i, mul_j, add_j in ((1, 0, 1, 0), (1, 17, 5, 3), (7, 40, 1, 64), (5, 1, 11, 95), (11, 33, 7, 31), (13, 64, 13, 0),
                                       (95, 95, 1, 32), (1, 32, 95, 63)):
        b = np.arange(n)
        i, j = (mul_i * b + add_i) % n, (mul_j * b + add_j) % n
        w_pos, w_neg = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
        w_pos[b, i], w_neg[b, j] = 1, 1
        got = _pairs(dev, s_pos, s_neg, w_pos, w_neg)
        want = torch.from_numpy(G[i, j])
        assert torch.equal(got, want), (mul_i, add_i, mul_j, add_j, torch.nonzero(got != want).flatten().tolist())
        seen_i |= set(zip(b.tolist(), i.tolist()))
        seen_j |= set(zip(b.tolist(), j.tolist()))
    for axis in (seen_i, seen_j):
        assert {v for _, v in axis} == set(range(n)) and {b for b, _ in axis} == set(range(n))
    # one replicate of the middle block alone, on pairs at the edges of the blocks: every other replicate stays 0
    for i0, j0 in ((32, 63), (63, 32), (0, 95), (95, 0), (31, 64), (64, 31)):
        w_pos, w_neg = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
        w_pos[40, i0], w_neg[40, j0] = 1, 1
        want = torch.zeros(n, dtype=torch.int64)
        want[40] = int(G[i0, j0])
        assert torch.equal(_pairs(dev, s_pos, s_neg, w_pos, w_neg), want), (i0, j0)


@pytest.mark.parametrize("kind", ("ties", "normal"))
@pytest.mark.parametrize("shape", ((1, 1, 1), (31, 33, 1), (32, 32, 32), (33, 65, 33), (70, 300, 37), (96, 1000, 65)))
def test_random_weights_are_exact(dev, shape, kind):
    """Weights random in [0, 127], no two replicates and no two positions alike; integer scores with plenty of ties (-0.0 against
    +0.0 among them) and normal fp32 scores, which are just as exact because only comparisons are made."""
    P, Nn, B = shape
    g = np.random.default_rng(P * 1000 + Nn)
    s_pos, s_neg = _scores(kind, P, P), _scores(kind, Nn, Nn + 7)
    if kind == "ties" and P > 1:
        s_pos[0], s_neg[0] = np.float32(-0.0), np.float32(0.0)
    w_pos, w_neg = g.integers(0, 128, (B, P)), g.integers(0, 128, (B, Nn))
    got = _pairs(dev, s_pos, s_neg, w_pos, w_neg)
    want = torch.from_numpy(A.u2(s_pos, s_neg, w_pos, w_neg))
    assert torch.equal(got, want), torch.nonzero(got != want).flatten().tolist()


def test_an_accumulator_beyond_2_pow_24_is_exact(dev):
    """P = 32, Nn = 66100, B = 1, all weights 127, every positive above every negative: T = 2 * 127 * 66100 = 16 789 400 > 2^24 per
    row, which an fp32 accumulation cannot hold."""
    P, Nn = 32, 66100
    got = _pairs(dev, np.ones(P, np.float32), np.zeros(Nn, np.float32), np.full((1, P), 127), np.full((1, Nn), 127))
    T = 2 * 127 * Nn
    assert T > 2 ** 24 and got.tolist() == [P * 127 * T]


def test_split_launches_equal_one_launch_and_runs_repeat(dev):
    """(96, 300, 37): the positives as one launch, as three launches of 32 / 40 / 24 rows at their offsets, and once more."""
    P, Nn, B = 96, 300, 37
    g = np.random.default_rng(8)
    s_pos, s_neg = _scores("ties", P, 3), _scores("ties", Nn, 4)
    w_pos, w_neg = g.integers(0, 128, (B, P)), g.integers(0, 128, (B, Nn))
    one = _pairs(dev, s_pos, s_neg, w_pos, w_neg)
    again = _pairs(dev, s_pos, s_neg, w_pos, w_neg)
    parts = sum(_pairs(dev, s_pos, s_neg, w_pos, w_neg, rows=r) for r in ((0, 32), (32, 72), (72, 96)))
    assert torch.equal(one, again) and torch.equal(one, parts) and torch.equal(one, torch.from_numpy(A.u2(s_pos, s_neg, w_pos, w_neg)))


@pytest.mark.parametrize("n,B,b0", [(n, 33, b0) for n in (1, 37, 300, 5000) for b0 in (0, 7)] + [(8200, 3, 2)])
def test_bootstrap_weights_equal_the_numpy_restatement(dev, n, B, b0):
    """(8200 crosses the kernel's tile of 8192 targets.)  The row stride is 16 beyond the padded width: every padding column is 0."""
    from mmgclip._hip import call, ptr, stream
    ld = (n + 15) // 16 * 16 + 16
    w = torch.full((B + 2, ld), 99, device=dev, dtype=torch.int8)
    w[:B] = -77
    call("mmg_bootstrap_weights", SEED, n, b0, B, ptr(w), ld, stream())
    torch.cuda.synchronize()
    assert bool((w[B:] == 99).all()), "a row after the last replicate was written"
    got = w[:B].cpu()
    assert torch.equal(got[:, :n].to(torch.int64), torch.from_numpy(A.weights(SEED, n, b0, B)))
    assert bool((got[:, n:] == 0).all())


def test_backend_and_metric_on_the_device_equal_the_reference(dev):
    """150 samples fed as 64 / 64 / 22, a binary and a 4-class task, 64 replicates: the dict equals the reference's; chunked the same."""
    from mmgclip import head, zeroshot_auroc
    tasks = A.example_tasks(150)
    want = A.reference(tasks, 64, SEED)
    w = head._HipAurocBackend.bootstrap_weights(SEED, 150, 3, 5, dev)
    assert w.shape == (5, 160) and torch.equal(w[:, :150].cpu().to(torch.int64), torch.from_numpy(A.weights(SEED, 150, 3, 5)))
    for cap in (64 << 20, 7 * 672):              # all 64 replicates at once, then 7 at a time
        z = zeroshot_auroc.ZeroShotAUROC(n_bootstrap=64, seed=SEED, max_weight_bytes=cap)
        for name, (scores, targets, values) in tasks.items():
            for a in range(0, 150, 64):
                z.update(name, torch.from_numpy(scores[a:a + 64]).to(dev), torch.from_numpy(targets[a:a + 64]).to(dev), values)
        got = z.compute()
        assert got == want
    print(got["malig"])
    m = got["malig"]
    assert m["n_valid"] == 64 and 0.5 < m["ci_lower"] <= m["auc"] <= m["ci_upper"] <= 1.0
    heavy = 8_500_000                      # 2 * 127 * 8 500 000 = 2 159 000 000 >= 2^31: refused on the host, nothing launched
    assert heavy % 16 == 0 and 2 * 127 * heavy >= 2 ** 31 > 2 * 127 * (heavy - 100_000)
    with pytest.raises(ValueError, match="2\\^31"):
        head._HipAurocBackend.pairs(torch.zeros(1, device=dev), torch.zeros(heavy, device=dev),
                                    torch.ones((1, 16), dtype=torch.int8, device=dev),
                                    torch.full((1, heavy), 127, dtype=torch.int8, device=dev))


def test_validate_fills_zeroshot_and_returns_the_same_tuple(dev, tmp_path, monkeypatch):
    """One validate() of a tiny model with the shipped example selected: `self.zeroshot` has the expected names and finite values,
    the malignancy AUROC equals the host's on the same scores; the same weights without the key return an equal 5-tuple."""
    from tests.test_retrieval_gpu import _experiment
    metrics = "experiments.config.metrics=[BenignMalignantDatasetLabels,MassShapeLabels,birads]"
    with_key = _experiment(monkeypatch, tmp_path, [metrics, "+experiments/config/zeroshot_auroc=bootstrap",
                                                   "experiments.config.zeroshot_auroc.n_bootstrap=64"])
    val = with_key.validate()
    torch.cuda.synchronize()
    z = with_key.zeroshot
    print(z["malig"], val)
    assert list(z) == ["birads", "malig", "shapes"]
    assert list(z["malig"]["classes"]) == [1] and list(z["shapes"]["classes"]) == [0, 1, 2, 3] and list(z["birads"]["classes"]) == list(range(-1, 7))
    m = z["malig"]
    assert set(m) == {"auc", "n_classes", "ci_mean", "ci_lower", "ci_upper", "n_valid", "classes"}
    assert all(np.isfinite(m[k]) for k in m if k != "classes") and m["classes"][1]["n_pos"] + m["classes"][1]["n_neg"] == 32
    assert 0.0 <= m["ci_lower"] <= m["ci_upper"] <= 1.0 and 0 < m["n_valid"] <= 64
    for name, at in (("malig", 1), ("shapes", 2), ("birads", 3)):
        assert z[name]["n_classes"] > 0 and abs(z[name]["auc"] - val[at]) <= 1e-12, (name, z[name]["auc"], val[at])
    without = _experiment(monkeypatch, tmp_path, [metrics])
    without.model.load_state_dict(with_key.model.state_dict())
    val2 = without.validate()
    assert without.zeroshot is None
    assert len(val) == 5 and all(np.isfinite(v) for v in val) and val == val2, (val, val2)
