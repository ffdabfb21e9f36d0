"""The reference of tests/auroc_ref.py is the reference project's bootstrap loop: its weighted pair count equals sklearn's
roc_auc_score on the resampled arrays (ties included) and its interval equals `Evaluator.calculate_ci` over those values; the draws
have the statistics of a bootstrap; a count above 127 raises; and the torch emulation the CPU tests run on agrees with the reference
exactly on cases that every listed mutation of it fails."""
import numpy as np
import pytest
import torch

from tests import auroc_ref as A

SEED = 11
# (n, B, kind): small on purpose - at n = 6 replicates with one class only occur, 37 and 50 are no multiple of 16
CASES = ((6, 40, "ties"), (37, 24, "ties"), (50, 16, "normal"), (33, 20, "ties"))


def _case(n, kind, seed):
    g = np.random.default_rng(seed)
    y = g.random(n) < 0.35
    y[0], y[1] = True, False
    s = A.tie_scores(n, seed) + (2 * y if n > 6 else 0) if kind == "ties" else g.standard_normal(n) + y
    return s.astype(np.float32), y


def test_the_weighted_form_is_the_bootstrap_loop_of_the_reference():
    """roc_auc_score on the resampled arrays, replicate by replicate, to 1e-12; one-class replicates are the ones left out; the CI
    of the case equals calculate_ci over sklearn's values."""
    from sklearn import metrics

    from mmgclip.evaluator import Evaluator
    for n, B, kind in CASES:
        s, y = _case(n, kind, n)
        ours = A.replicate_aucs(s, y, SEED, B)
        theirs = []
        for b in range(B):
            idx = A.draws(SEED, n, b)
            theirs.append(metrics.roc_auc_score(y[idx], s[idx]) if len(np.unique(y[idx])) == 2 else None)
        assert [v is None for v in ours] == [v is None for v in theirs]
        assert all(abs(a - t) <= 1e-12 for a, t in zip(ours, theirs) if a is not None)
        valid = [t for t in theirs if t is not None]
        mean, lo, hi = Evaluator.calculate_ci(None, valid)
        got = A.calculate_ci([v for v in ours if v is not None])
        assert abs(got[0] - mean) <= 1e-12 and abs(got[1] - lo) <= 1e-12 and abs(got[2] - hi) <= 1e-12 and got[3] == len(valid)
    assert any(v is None for v in A.replicate_aucs(*_case(6, "ties", 6), SEED, 40)), "the n = 6 case must contain one-class replicates"
    # the point estimate is the replicate whose weights are all 1
    s, y = _case(37, "ties", 37)
    point = int(A.u2(s[y], s[~y], np.ones((1, y.sum())), np.ones((1, (~y).sum())))[0]) / (2 * int(y.sum()) * int((~y).sum()))
    assert abs(point - metrics.roc_auc_score(y, s)) <= 1e-12


def test_signed_zeros_tie():
    assert A.g_matrix(np.float32([-0.0, 0.0, 1.0]), np.float32([0.0, -0.0])).tolist() == [[1, 1], [1, 1], [2, 2]]


def test_draw_statistics():
    """Every replicate's weights sum to n; at n = 16384 about 1/e of them are zero; the draw is a pure function of (seed, b)."""
    for n in (1, 37, 300, 16384):
        w = A.weights(SEED, n, 0, 8)
        assert w.shape == (8, n) and (w.sum(axis=1) == n).all() and w.min() >= 0 and w.max() <= 127
    w = A.weights(SEED, 16384, 0, 8)
    assert 0.36 <= (w == 0).mean() <= 0.375, (w == 0).mean()
    assert np.array_equal(A.weights(SEED, 300, 5, 3), A.weights(SEED, 300, 0, 8)[5:8])
    assert not np.array_equal(A.weights(SEED, 300, 0, 1), A.weights(SEED + 1, 300, 0, 1))
    assert not np.array_equal(A.weights(SEED, 300, 0, 1), A.weights(SEED, 300, 1, 1))


def test_a_count_above_127_raises(monkeypatch):
    from mmgclip import head, zeroshot_auroc
    monkeypatch.setattr(head, "_HipAurocBackend", A.emulation(patched_draw=lambda seed, n, b: np.zeros(n, dtype=np.int64)))
    s, y = _case(200, "ties", 1)
    z = zeroshot_auroc.ZeroShotAUROC(n_bootstrap=4, seed=SEED)
    z.update("t", torch.from_numpy(s)[:, None], torch.from_numpy(y.astype(np.int64)), [1])
    with pytest.raises(OverflowError, match="127"):
        z.compute()
    with pytest.raises(OverflowError):
        A.emulated_replicate_aucs(A.emulation(patched_draw=lambda seed, n, b: np.zeros(n, dtype=np.int64)), s, y, SEED, 4)
    # 127 itself is a count like any other
    w = A.emulation(patched_draw=lambda seed, n, b: np.zeros(127, dtype=np.int64)).bootstrap_weights(SEED, 127, 0, 1)
    assert int(w[0, 0]) == 127 and int(w.sum()) == 127


def _emulated(mutation):
    be = A.emulation(mutation if mutation != "one_class_replicate_kept" else None)
    return [A.emulated_replicate_aucs(be, *_case(n, kind, n), SEED, B, keep_one_class=mutation == "one_class_replicate_kept")
            for n, B, kind in CASES]


def test_the_emulation_equals_the_reference_on_the_exact_cases():
    want = [A.replicate_aucs(*_case(n, kind, n), SEED, B) for n, B, kind in CASES]
    assert _emulated(None) == want


@pytest.mark.parametrize("mutation", A.MUTATIONS)
def test_every_mutation_fails_an_exact_case(mutation):
    want = [A.replicate_aucs(*_case(n, kind, n), SEED, B) for n, B, kind in CASES]
    got = _emulated(mutation)
    assert any(g != w for g, w in zip(got, want)), f"the exact cases do not see the mutation {mutation}"
