"""tests/retrieval_ref.py checked on the CPU before anything relies on it: the reference against a dense argsort-based ranking under
the same tie convention, the metric formulas against plain float64 torch, the preconditions of both regimes on the reference alone,
and every mutation of the emulation caught by at least one exact case."""
import pytest
import torch

from tests import retrieval_ref as R

ABSENT_CASE = ((40, 300, 64, 0), 5)           # the labelled case that carries a query whose key is absent from the gallery


def _case(shape, mode, regime):
    n, N, D, off = shape
    X, Y = R.exact_case(n, N, D, off) if regime == "exact" else R.gaussian_case(n, N, D, seed=7 * N + D)
    absent = ABSENT_CASE[1] if (regime == "exact" and mode == "labels" and shape == ABSENT_CASE[0]) else None
    key, lab = R.keys_for(mode, n, N, off, absent)
    return X, Y, key, lab, R.positive_mask(n, N, off, key, lab)


def dense_ranks(X, Y, pos):
    """The independent statement: sort every query's gallery by descending score with, among equal scores, negatives BEFORE
    positives (ties count against the model); the rank is one more than the number of negatives in front of the first positive."""
    s = X.double() @ Y.double().t()
    ranks = []
    for i in range(s.shape[0]):
        if not bool(pos[i].any()):
            ranks.append(None)
            continue
        order = torch.argsort(pos[i].long(), stable=True)                       # negatives first ...
        order = order[torch.argsort(-s[i][order], stable=True)]                # ... inside every run of equal scores
        where = int(torch.nonzero(pos[i][order])[0])
        ranks.append(1 + int((~pos[i][order][:where]).sum()))
    return ranks


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.EXACT_SHAPES)
def test_reference_is_the_dense_argsort_ranking(shape, mode):
    X, Y, _, _, pos = _case(shape, mode, "exact")
    r = R.reference(X, Y, pos)
    want = dense_ranks(X, Y, pos)
    got = [int(v) if int(p) > 0 else None for v, p in zip(r.rank, r.n_pos)]
    assert got == want
    none = r.n_pos == 0
    assert bool((r.best[none] == float("-inf")).all()) and torch.equal(r.n_gt[none], torch.full_like(r.n_gt[none], shape[1]))
    assert torch.equal(r.n_eq[none], torch.zeros_like(r.n_eq[none]))


def test_the_absent_key_case_has_a_query_without_positives_and_ties_are_plentiful():
    shape, row = ABSENT_CASE
    X, Y, key, lab, pos = _case(shape, "labels", "exact")
    r = R.reference(X, Y, pos)
    assert int(r.n_pos[row]) == 0 and float(r.best[row]) == float("-inf") and int(r.n_gt[row]) == shape[1] and int(r.n_eq[row]) == 0
    assert int((r.n_pos == 0).sum()) == 1
    for shape in R.EXACT_SHAPES[1:]:
        for mode in R.MODES:
            X, Y, _, _, pos = _case(shape, mode, "exact")
            r = R.reference(X, Y, pos)
            assert int((r.n_eq > 0).sum()) >= 1, (shape, mode)                   # `>=` for `>` cannot pass
            assert int((r.n_gt > 0).sum()) >= 1 or shape[1] < 32, (shape, mode)


@pytest.mark.parametrize("shape", R.EXACT_SHAPES)
def test_exact_regime_preconditions(shape):
    X, Y = R.exact_case(*shape)
    assert R.exactness_violations(X, Y) == []
    s = X.double() @ Y.double().t()
    assert float(s.abs().max()) <= 4 * shape[2] <= 4096 and torch.equal(s, s.round())
    assert torch.equal((X @ Y.t()).double(), s)                                   # fp32 forms it exactly
    assert R.exactness_violations(X + 0.5, Y) != [] and R.exactness_violations(X, 3 * Y.abs() + 1) != []


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.GAUSS_SHAPES)
def test_gaussian_intervals_are_mostly_points_and_hold_the_emulation(shape, mode):
    """The 1/8 cap on open intervals, on the reference alone; then the fp32 emulation (an honest fp32 computation) inside every
    interval, and a count moved by one outside."""
    X, Y, key, lab, pos = _case(shape, mode, "gauss")
    r = R.intervals(X, Y, pos)
    print(shape, mode, "open share", r.open_share)
    assert r.open_share <= R.OPEN_CAP
    assert bool((r.lo <= r.n_gt).all()) and bool((r.n_gt + r.n_eq <= r.hi).all())
    got = R.emulate(X, Y, key, lab, shape[3])
    assert R.interval_violations(r, *got) == []
    best, n_pos, n_gt, n_eq = got
    row = int(torch.nonzero(r.lo == r.hi)[0])
    bumped = n_gt.clone()
    bumped[row] += 1
    assert R.interval_violations(r, best, n_pos, bumped, n_eq) != []
    assert R.interval_violations(r, best + 1e-3, n_pos, n_gt, n_eq) != []


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_fails_an_exact_case(mut):
    caught = []
    for shape in R.EXACT_SHAPES:
        for mode in R.MODES:
            X, Y, key, lab, pos = _case(shape, mode, "exact")
            r = R.reference(X, Y, pos)
            want = (r.best.float(), r.n_pos.int(), r.n_gt.int(), r.n_eq.int())
            assert all(torch.equal(a, b) for a, b in zip(R.emulate(X, Y, key, lab, shape[3]), want)), (shape, mode)
            if not all(torch.equal(a, b) for a, b in zip(R.emulate(X, Y, key, lab, shape[3], mut=mut), want)):
                caught.append((shape, mode))
    print(mut, caught)
    assert caught, f"no exact case notices {mut}"


@pytest.mark.parametrize("labelled", [False, True])
def test_metric_formulas_against_plain_torch(labelled):
    img, txt, _, group = R.exact_pairs(150, 64)
    labels = group if labelled else None
    m = R.reference_metrics(img, txt, labels, ks=(1, 5, 10))
    pos = R.positive_mask(150, 150, 0, labels, labels)
    for name, x, y in (("i2t", img, txt), ("t2i", txt, img)):
        rank = torch.tensor(dense_ranks(x, y, pos)).double()
        for k in (1, 5, 10):
            assert m[f"{name}_R@{k}"] == float((rank <= k).double().mean())
        assert m[f"{name}_median_rank"] == float(torch.quantile(rank, 0.5))
        assert m[f"{name}_mrr"] == pytest.approx(float((1.0 / rank).mean()), rel=1e-13)
        assert m[f"{name}_n_queries"] == 150 and m[f"{name}_no_positive"] == 0 and 0.0 < m[f"{name}_ties"] < 1.0
    assert set(m) == {f"{d}_{k}" for d in ("i2t", "t2i") for k in ("R@1", "R@5", "R@10", "median_rank", "mrr", "ties", "n_queries", "no_positive")}
    if labelled:                     # duplicates of the right report stop counting against the model
        plain = R.reference_metrics(img, txt, None, ks=(1, 5, 10))
        assert m["i2t_R@1"] > plain["i2t_R@1"] and m["i2t_mrr"] > plain["i2t_mrr"]


def test_a_collapsed_model_scores_zero_not_one():
    ones = torch.ones(40, 32)
    m = R.reference_metrics(ones, ones, None, ks=(1, 5, 10))
    assert m["i2t_R@1"] == m["t2i_R@10"] == 0.0 and m["i2t_median_rank"] == 40.0 and m["i2t_ties"] == 1.0 and m["i2t_mrr"] == 1.0 / 40
