"""tests/sigmoid_ref.py checked on the CPU: the float64 reference against an independent statement, the exactness preconditions on
the reference alone, the fp32 emulation of the kernels inside every bar (exact where the table says exact) and every mutation of it
outside them on every case that contains the mutated feature."""
import math

import pytest
import torch

from tests import sigmoid_ref as R

MUT_SB = (10.0, -3.0)      # the mutation table's scalars: negatives near softplus(-3) = 0.05, far above every bar


@pytest.mark.parametrize("mode", R.MODES)
def test_reference_agrees_with_the_independent_statement(mode):
    """-logsigmoid(y z).sum() / N with float64 autograd, both positives modes, to 1e-12."""
    for N, D, (s, b) in ((37, 64, R.SB_PAIRS[0]), (70, 32, R.SB_PAIRS[1]), (33, 96, R.SB_PAIRS[2])):
        img, txt = R.gaussian_case(N, N, D, seed=N)
        labels = None if mode == "diagonal" else R.hand_labels(N)
        s, b = R.f32(s), R.f32(b)
        ref = R.reference_loss(img, txt, s, b, labels)
        loss, dimg, dtxt, ds, db = R.pinned_statement(img, txt, s, b, labels)
        for got, want in ((ref.loss, loss), (ref.dimg, dimg), (ref.dtxt, dtxt), (ref.dscale, ds), (ref.dbias, db)):
            got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        assert float(ref.row_loss.sum() / N - loss) == pytest.approx(0.0, abs=1e-12 * float(loss))


def test_hand_labels_hold_a_seam_cluster_and_a_singleton():
    for N in (33, 65, 96, 129):
        lab = R.hand_labels(N)
        assert int((lab == lab[0]).sum()) == 1                                   # the singleton
        assert len({int(lab[j]) for j in range(30, 34 if N > 33 else N)}) == 1    # one cluster on both sides of column 32
        assert lab.tolist() == sorted(lab.tolist()) and int(lab.max()) + 1 == len(set(lab.tolist()))


def _case(shape, mode, sb, exact, coef, gout, ds0, db0, mut=None):
    n, N, D, off = shape
    if exact:
        X, Y, key, lab = R.exact_case(n, N, D, off, mode == "clusters")
        s, b = R.EXACT_S, R.EXACT_B
    else:
        X, Y = R.gaussian_case(n, N, D, seed=7 * N + D)
        key, lab = R.keys_for(mode, n, N, off)
        s, b = R.f32(sb[0]), R.f32(sb[1])
    pos = R.positive_mask(n, N, off, key, lab)
    ref = R.reference(X, Y, s, b, pos, coef, 1.0 if gout is None else gout, ds0, db0)
    got = R.emulate(X, Y, s, b, key, lab, off, coef, gout, ds0, db0, mut=mut)
    return ref, got, pos


def _ratios(ref, got):
    row_loss, dX, ds, db = got
    return dict(row_loss=R.ratio(row_loss, ref.row_loss, ref.E_row_loss), dX=R.ratio(dX, ref.dX, ref.E_dX),
                dscale=R.ratio(ds, ref.dscale, ref.E_dscale), dbias=R.ratio(db, ref.dbias, ref.E_dbias))


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_emulation_is_inside_every_bar(shape, mode):
    for sb in R.SB_PAIRS + (MUT_SB,):
        for gout in (None, 0.25):
            ref, got, _ = _case(shape, mode, sb, False, R.f32(1.0 / shape[1]), gout, 0.5, -3.0)
            q = _ratios(ref, got)
            assert max(q.values()) <= 1.0, (sb, gout, q)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_exact_regime_preconditions_and_emulation(shape, mode):
    """On the reference alone: |z| = 128 for every pair, both kinds of pair misclassified, every output a dyadic sum below 2^24 units.
    The emulation then reproduces the reference bit for bit."""
    coef = 2.0 ** -math.ceil(math.log2(shape[1]))
    for gout in (None, 0.25):
        ref, got, pos = _case(shape, mode, None, True, coef, gout, 0.5, -3.0)
        assert R.exactness_violations(ref, pos, coef, 1.0 if gout is None else gout, 0.5, -3.0) == []
        assert bool(((ref.sp < 1e-50) | (ref.sp == 128)).all()) and bool(((ref.g.abs() < 1e-50) | (ref.g.abs() == coef * (gout or 1.0))).all())
        row_loss, dX, ds, db = got
        assert torch.equal(row_loss, ref.row_loss.float()) and torch.equal(dX, ref.dX.float())
        assert float(ds) == float(ref.dscale) and float(db) == float(ref.dbias)


def _contains(mut, shape, mode):
    """Does the case contain the feature the mutation breaks?  -> the outputs that must leave their bars (None = not contained)."""
    n, N, D, off = shape
    return {"no_bias": ("row_loss", "dbias"),
            "pos_sign": ("row_loss", "dbias"),
            "no_diag_off": ("row_loss",) if (mode == "diagonal" and off != 0) else None,
            "label_vs_index": ("row_loss",) if (mode == "clusters" and N > 1) else None,
            "pad_col": ("row_loss", "dbias") if N % 32 else None,
            "pad_row": ("dscale", "dbias") if n % 32 else None,
            "no_coef_dbias": ("dbias",),
            "naive_softplus": None}[mut]


@pytest.mark.parametrize("mut", [m for m in R.MUTATIONS if m != "naive_softplus"])
def test_every_mutation_leaves_the_bars(mut):
    seen = 0
    for shape in R.SHAPES:
        for mode in R.MODES:
            outs = _contains(mut, shape, mode)
            if outs is None:
                continue
            ref, got, _ = _case(shape, mode, MUT_SB, False, R.f32(1.0 / shape[1]) if shape[1] > 1 else 0.5, 0.25, 0.5, -3.0, mut=mut)
            q = _ratios(ref, got)
            assert all(q[o] > 1.0 for o in outs), (mut, shape, mode, q)
            seen += 1
    assert seen >= 1


@pytest.mark.parametrize("mode", R.MODES)
def test_naive_softplus_leaves_the_bars_where_u_is_large(mode):
    """log(1 + exp(u)) overflows at u = 128: the feature is a large positive u, which every case of the exact regime contains (each
    has a misclassified pair).  (At large negative u the naive form returns log(1) = 0, an absolute error below exp(u) that no
    row sum holding a positive pair can show.)"""
    for shape in R.SHAPES:
        ref, got, _ = _case(shape, mode, None, True, 2.0 ** -8, None, 0.5, -3.0, mut="naive_softplus")
        assert _ratios(ref, got)["row_loss"] > 1.0, shape


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("world", [1, 2, 4])
def test_host_choreography_emulated_and_mutated(world, mode):
    """emulate_loss over simulated ranks against the unsharded float64 reference; the scalars counted by both launches and the
    normalisation by n_loc leave the bars (the latter wherever n_loc != N)."""
    N, D = 64, 32
    img, txt = R.gaussian_case(N, N, D, seed=3)
    labels = None if mode == "diagonal" else R.hand_labels(N)
    s, b = R.f32(MUT_SB[0]), R.f32(MUT_SB[1])
    ref = R.reference_loss(img, txt, s, b, labels, gout=0.25, ranks=world)

    def q(out):
        loss, dimg, dtxt, ds, db = out
        return dict(loss=R.ratio(loss, ref.loss, ref.E_loss), dimg=R.ratio(dimg, ref.dimg, ref.E_dimg), dtxt=R.ratio(dtxt, ref.dtxt, ref.E_dtxt),
                    dscale=R.ratio(ds, ref.dscale, ref.E_dscale), dbias=R.ratio(db, ref.dbias, ref.E_dbias))
    good = q(R.emulate_loss(img, txt, s, b, labels, world, 0.25))
    assert max(good.values()) <= 1.0, good
    twice = q(R.emulate_loss(img, txt, s, b, labels, world, 0.25, mut="scalars_twice"))
    assert twice["dscale"] > 1.0 and twice["dbias"] > 1.0, twice
    if world > 1:
        norm = q(R.emulate_loss(img, txt, s, b, labels, world, 0.25, mut="norm_n_loc"))
        assert norm["loss"] > 1.0 and norm["dimg"] > 1.0 and norm["dbias"] > 1.0, norm
