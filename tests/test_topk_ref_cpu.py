"""tests/topk_ref.py checked on the CPU before anything relies on it: the reference against a dense per-row argsort written here, the
preconditions of both regimes on the reference alone, the emulation against the reference (exact: torch.equal; Gaussian: inside the
intervals), every mutation caught by at least one exact case, chunked against one pass, and `search.merge_topk` against the reference
on concatenated candidate lists."""
import os
import sys

import pytest
import torch

from tests import topk_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paths():
    for p in (ROOT, os.path.join(ROOT, "mmg-clip_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


def dense_topk(X, Y, k, excluded, j_base=0):
    """The independent statement: per row, the admissible columns sorted by (-score, index) as Python tuples."""
    s = (X.double() @ Y.double().t()).tolist()
    scores, indices = [], []
    for i, row in enumerate(s):
        cand = sorted((-v, j) for j, v in enumerate(row) if not bool(excluded[i, j]))[:k]
        scores.append([-v for v, _ in cand] + [T.NINF] * (k - len(cand)))
        indices.append([j + j_base for _, j in cand] + [-1] * (k - len(cand)))
    return torch.tensor(scores, dtype=torch.float64).reshape(len(s), k), torch.tensor(indices, dtype=torch.int64).reshape(len(s), k)


def _want(r):
    return r.scores.float(), r.indices.int()


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("shape", T.EXACT_SHAPES)
def test_reference_is_the_dense_argsort(shape, mode):
    X, Y, _, _, excluded = T.case(shape, mode, "exact")
    for j_base in (0, 1000):
        r = T.reference(X, Y, shape[4], excluded, j_base)
        scores, indices = dense_topk(X, Y, shape[4], excluded, j_base)
        assert torch.equal(r.scores, scores) and torch.equal(r.indices, indices)


def test_the_exact_cases_have_ties_padding_and_a_query_that_excludes_nothing():
    shape, row = T.ABSENT_CASE
    X, Y, key, lab, excluded = T.case(shape, "labels", "exact")
    assert int(excluded[row].sum()) == 0 and int((excluded.sum(1) == 0).sum()) == 1 and bool((excluded.sum(1) > 1).any())
    Xs, Ys, _, _, ex = T.case((3, 5, 32, 0, 8), "diagonal", "exact")          # k > N: four admissible columns, four padding slots
    r = T.reference(Xs, Ys, 8, ex)
    assert torch.equal(r.n_adm, torch.full((3,), 4)) and bool((r.indices[:, 4:] == -1).all()) and bool((r.scores[:, 4:] == T.NINF).all())
    for shape in T.EXACT_SHAPES[2:]:                              # a tie INSIDE the list and one ACROSS its end: only the index decides
        X, Y, _, _, excluded = T.case(shape, "none", "exact")
        k = shape[4]
        r = T.reference(X, Y, k + 1, excluded)
        assert bool((r.scores[:, :k - 1] == r.scores[:, 1:k]).any()) or k == 1, shape
        assert bool((r.scores[:, k - 1] == r.scores[:, k]).any()), shape


@pytest.mark.parametrize("shape", T.EXACT_SHAPES)
def test_exact_regime_preconditions(shape):
    X, Y = T.exact_case(*shape[:4])
    assert T.exactness_violations(X, Y) == []
    s = X.double() @ Y.double().t()
    assert float(s.abs().max()) <= 4 * shape[2] <= 4096 and torch.equal(s, s.round())
    assert torch.equal((X @ Y.t()).double(), s)                                   # fp32 forms it exactly
    assert T.exactness_violations(X + 0.5, Y) != [] and T.exactness_violations(X, 3 * Y.abs() + 1) != []
    assert T.supported(shape[2], shape[4])


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("shape", T.EXACT_SHAPES)
def test_emulation_equals_the_reference_on_exact_cases(shape, mode):
    X, Y, key, lab, excluded = T.case(shape, mode, "exact")
    n, N, D, off, k = shape
    want = _want(T.reference(X, Y, k, excluded))
    got = T.emulate(X, Y, k, T.EXCLUDE[mode], key, lab, off)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("shape", T.EXACT_SHAPES)
def test_chunked_emulation_equals_one_pass(shape, mode):
    """Three uneven chunks through j_base / accumulate (fewer where N < 3)."""
    X, Y, key, lab, excluded = T.case(shape, mode, "exact")
    n, N, D, off, k = shape
    one = T.emulate(X, Y, k, T.EXCLUDE[mode], key, lab, off)
    cuts = T.three_cuts(N)
    assert len(cuts) == min(3, N) and all(b > a for a, b in cuts) and (len({b - a for a, b in cuts}) > 1 or N == 1)
    got = T.emulate_chunked(X, Y, k, T.EXCLUDE[mode], key, lab, off, cuts)
    assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])
    assert all(torch.equal(a, b) for a, b in zip(got, _want(T.reference(X, Y, k, excluded))))


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("shape", T.GAUSS_SHAPES)
def test_gaussian_intervals_are_mostly_decided_and_hold_the_emulation(shape, mode):
    """The 1/8 cap on open rows, on the reference alone; then the fp32 emulation (an honest fp32 computation) passes every check, and
    lists that are wrong in one place do not."""
    X, Y, key, lab, excluded = T.case(shape, mode, "gauss")
    n, N, D, off, k = shape
    r = T.intervals(X, Y, k, excluded)
    print(shape, mode, "open share", r.open_share, "decided rows", int(r.decided.sum()), "of", n)
    assert r.open_share <= T.OPEN_CAP
    assert int(r.decided.sum()) >= n // 2
    assert T.interval_violations(r, r.scores.float(), r.indices.int()) == []      # the reference passes its own checks
    scores, indices = T.emulate(X, Y, k, T.EXCLUDE[mode], key, lab, off)
    assert T.interval_violations(r, scores, indices) == []
    row = int(torch.nonzero(~r.open_rows & r.decided)[0])
    m = min(k, int(r.n_adm[row]))
    swapped = indices.clone()
    # a column that cannot be there: surely out, or (where k takes every admissible column) an excluded one
    outsider = next(j for j in range(N) if bool(r.sure_out[row, j] if m < int(r.n_adm[row]) else excluded[row, j]))
    swapped[row, m - 1] = outsider
    assert T.interval_violations(r, scores, swapped) != []
    assert T.interval_violations(r, scores + 1e-3, indices) != []
    if m >= 2:
        flipped_s, flipped_j = scores.clone(), indices.clone()
        flipped_s[row, :2], flipped_j[row, :2] = scores[row, :2].flip(0), indices[row, :2].flip(0)
        assert T.interval_violations(r, flipped_s, flipped_j) != []
        twice = indices.clone()
        twice[row, 1] = twice[row, 0]
        assert T.interval_violations(r, scores, twice) != []


@pytest.mark.parametrize("mut", T.MUTATIONS)
def test_every_mutation_fails_an_exact_case(mut):
    """Every exact shape and mode, in one pass and as three chunks: the clean emulation equals the reference, the mutated one does
    not somewhere."""
    caught = []
    for shape in T.EXACT_SHAPES:
        n, N, D, off, k = shape
        for mode in T.MODES:
            X, Y, key, lab, excluded = T.case(shape, mode, "exact")
            want = _want(T.reference(X, Y, k, excluded))
            for how, cuts in (("one pass", [(0, N)]), ("chunks", T.three_cuts(N))):
                got = T.emulate_chunked(X, Y, k, T.EXCLUDE[mode], key, lab, off, cuts, mut=mut)
                if not (got[0].shape == want[0].shape and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])):
                    caught.append((shape, mode, how))
    print(mut, len(caught), caught[:6])
    assert caught, f"no exact case notices {mut}"


def test_support_table_of_the_reference():
    for D in range(32, 1025, 32):
        for k in range(1, 33):
            if D <= 768 or k <= 16:
                assert T.supported(D, k) and T.lds_bytes(D, k) <= T.LDS_LIMIT, (D, k)
    assert not T.supported(1024, 32) and not T.supported(48, 4) and not T.supported(1056, 1) and not T.supported(64, 33) and not T.supported(64, 0)


@pytest.mark.parametrize("mode", T.MODES)
def test_merge_topk_equals_the_reference_on_concatenated_lists(mode):
    """The candidate lists of three column chunks, each padded and in any order, merged by `search.merge_topk`; a row with nothing
    admissible anywhere stays all padding."""
    _paths()
    from mmgclip.search import merge_topk
    shape = (40, 300, 64, 0, 32)
    n, N, D, off, k = shape
    X, Y, key, lab, excluded = T.case(shape, mode, "exact")
    excluded = excluded.clone()
    excluded[7] = True                                            # an all-padding row
    parts = []
    for a, b in T.three_cuts(N):
        r = T.reference(X, Y[a:b], k, excluded[:, a:b], a)
        parts.append((r.scores.float(), r.indices))
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(3 * k, generator=g)
    scores, indices = torch.cat([p[0] for p in parts], dim=1)[:, perm], torch.cat([p[1] for p in parts], dim=1)[:, perm]
    want = T.reference(X, Y, k, excluded)
    for kk in (k, 5, 1):
        got = merge_topk(scores, indices, kk)
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64
        assert torch.equal(got[0], want.scores.float()[:, :kk]) and torch.equal(got[1], want.indices[:, :kk])
    assert bool((want.indices[7] == -1).all()) and bool((want.scores[7] == T.NINF).all())
    wide = merge_topk(scores[:, :4], indices[:, :4], 6)           # fewer candidates than k: padded
    assert wide[0].shape == (n, 6) and bool((wide[1][:, 4:] == -1).all()) and bool((wide[0][:, 4:] == T.NINF).all())
    with pytest.raises(ValueError, match="candidate lists"):
        merge_topk(scores, indices[:, :5], 3)
