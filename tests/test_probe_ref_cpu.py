"""The yardsticks of the linear probe checked against things that are not ours (no GPU): the float64 reference gradient against torch
autograd of F; the product's L-BFGS over the reference evaluation against scipy's L-BFGS-B on the same F and against sklearn's
LogisticRegression(C = 1 / (l2 S)), within the distance strong convexity gives, ||W1 - W2|| <= (||g1|| + ||g2||) / l2 with both
gradients evaluated in float64; the exact cases' int64 expectations against the float64 reference; the fp32 emulation of the kernel's
partial structure inside the derived bar on the GPU test's shapes and bit-exact on its exact cases; every mutation of the emulation
outside; and the seeded blobs of the GPU fit test, which leave no row undecided at the reference optimum."""
import numpy as np
import pytest
import torch

from tests import probe_ref as P
from tests.test_averaged_fused_cpu import _paths


def _inside(got, want, bar):
    return bool(((got - want).abs() <= bar).all())


@pytest.mark.parametrize("weighted", [False, True])
def test_reference_gradient_equals_autograd_of_the_objective(weighted):
    n, D, C, l2 = 97, 32, 5, 3e-2
    X, W, b, y, cw = P.random_case(n, D, C, seed=3)
    cw = cw if weighted else None
    theta = torch.cat([W, b[:, None]], dim=1).double().flatten().requires_grad_(True)
    t = theta.reshape(C, D + 1)
    z = X.double() @ t[:, :D].t() + t[:, D]
    valid = y >= 0
    w = (torch.ones(n, dtype=torch.float64) if cw is None else cw.double()[y.clamp(min=0)]) * valid
    rows = torch.nn.functional.cross_entropy(z, y.clamp(min=0), reduction="none")
    F = (w * rows).sum() / w.sum() + 0.5 * l2 * (t[:, :D] ** 2).sum()
    F.backward()
    F = F.detach()
    f, g = P.objective(theta.detach().numpy(), X, y, C, l2, cw)
    assert abs(f - float(F)) <= 1e-13 * abs(float(F))
    assert np.abs(g - theta.grad.numpy()).max() <= 1e-13 * max(1.0, np.abs(g).max())
    assert w.sum().item() == P.weight_sum(y, cw)


def test_the_solver_reaches_the_optimum_of_scipy_and_sklearn():
    _paths()
    from scipy.optimize import minimize
    from sklearn.linear_model import LogisticRegression
    n, D, C, l2 = P.BLOBS["n"], P.BLOBS["D"], P.BLOBS["C"], P.BLOBS["l2"]
    X, y = P.blobs()
    ours, f, g, n_iter, converged, n_eval = P.reference_solver(X, y, C, l2, max_iter=500, gtol=1e-9)
    assert converged and n_iter < 500 and n_eval >= n_iter + 1
    fun = lambda th: P.objective(th, X, y, C, l2)                               # noqa: E731
    sp = minimize(fun, np.zeros(C * (D + 1)), jac=True, method="L-BFGS-B", options=dict(maxiter=5000, ftol=1e-16, gtol=1e-10))
    keep = (y >= 0).numpy()
    S = P.weight_sum(y)
    assert S == keep.sum()
    sk = LogisticRegression(C=1.0 / (l2 * S), tol=1e-10, max_iter=5000, solver="lbfgs").fit(X.double().numpy()[keep], y.numpy()[keep])
    theta_sk = np.concatenate([sk.coef_, sk.intercept_[:, None]], axis=1).reshape(-1)
    for name, other in (("scipy", sp.x), ("sklearn", theta_sk)):
        g_other = fun(other)[1]
        dist = np.linalg.norm((ours - other).reshape(C, D + 1)[:, :D])
        bound = P.convexity_distance(g, g_other, l2)
        print(name, "distance in W", dist, "bound", bound, "objective", f, fun(other)[0])
        assert dist <= bound, (name, dist, bound)
        assert bound < 1e-4, (name, bound)                                       # both really are at the optimum: the check has teeth


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [2, 4, 32])
def test_exact_expectations_equal_the_reference_and_the_emulation_is_bit_exact(C, weighted):
    D = 64
    for n in P.EXACT_NS:
        X, W, b, y, cw, dW, db = P.zero_weight_case(n, D, C, weighted)
        r = P.reference(X, W, b, y, cw)
        assert torch.equal(r["dW"], dW) and torch.equal(r["db"], db)             # int64 arithmetic = float64 arithmetic here
        Xs, Ws, bs, ys, cws, dWs, dbs, Ls = P.saturated_case(n, D, C, weighted)
        rs = P.reference(Xs, Ws, bs, ys, cws)
        # float64 still sees exp(-216) = 1e-94, which fp32 does not: one-hot up to that
        assert float((rs["dW"] - dWs).abs().max()) < 1e-80 and float((rs["db"] - dbs).abs().max()) < 1e-80
        assert abs(float(rs["L"]) - float(Ls)) < 1e-80 or abs(float(rs["L"]) - float(Ls)) <= 2.0 ** -52 * abs(float(Ls))
        gaps = rs["z"].topk(2, dim=1).values
        assert bool((gaps[:, 0] - gaps[:, 1] >= 200).all()) and bool((rs["z"] == rs["z"].round()).all())
        for groups in P.EXACT_GROUPS:
            out = P.emulate(X, W, b, y, cw, groups)
            assert torch.equal(out[:-1], P.flat(r["L"], dW, db)[:-1]), (n, groups)
            assert abs(float(out[-1]) - float(r["L"])) <= float(P.bar(X, W, b, y, cw, groups)[-1])
            outs = P.emulate(Xs, Ws, bs, ys, cws, groups)
            assert torch.equal(outs, P.flat(Ls, dWs, dbs)), (n, groups)
    assert bool((ys < 0).any()) and bool((y < 0).any())                           # ignore labels are part of the cases
    assert bool(((ys >= 0) & (Xs[:, :C].argmax(dim=1) != ys)).any())              # and so are misclassified rows


@pytest.mark.parametrize("shape", P.RANDOM_SHAPES)
def test_the_emulation_stays_inside_the_bar(shape):
    n, D, C = shape
    X, W, b, y, cw = P.random_case(n, D, C)
    r = P.reference(X, W, b, y, cw)
    want = P.flat(r["L"], r["dW"], r["db"])
    for groups in (0, 3):
        got = P.emulate(X, W, b, y, cw, groups)
        limit = P.bar(X, W, b, y, cw, groups)
        ratio = float(((got - want).abs() / limit).max())
        print(shape, "groups", groups, "worst |error| / bar", ratio, "bar of L relative", float(limit[-1] / want[-1].abs()))
        assert ratio <= 1.0
        # the bar is no blank cheque: a worst-case bound, yet below 1 % of the largest gradient entry everywhere
        assert float((limit[:-1] / (want[:-1].abs() + want[:-1].abs().max())).max()) < 1e-2


def _mutation_cases():
    cases = []
    for weighted in (False, True):
        X, W, b, y, cw, dW, db = P.zero_weight_case(33, 64, 4, weighted)
        cases.append((X, W, b, y, cw))
        cases.append(P.saturated_case(200, 64, 4, weighted)[:5])
    X, W, b, y, cw = P.random_case(257, 96, 3)
    cases.append((X, W, b, y, cw))
    return cases


def test_the_unmutated_emulation_passes_the_mutation_cases():
    for X, W, b, y, cw in _mutation_cases():
        r = P.reference(X, W, b, y, cw)
        assert _inside(P.emulate(X, W, b, y, cw, 3), P.flat(r["L"], r["dW"], r["db"]), P.bar(X, W, b, y, cw, 3))


@pytest.mark.parametrize("mutation", P.MUTATIONS)
def test_every_mutation_leaves_the_bar(mutation):
    assert len(P.MUTATIONS) >= 8
    failed = 0
    for X, W, b, y, cw in _mutation_cases():
        r = P.reference(X, W, b, y, cw)
        failed += not _inside(P.emulate(X, W, b, y, cw, 3, mut=mutation), P.flat(r["L"], r["dW"], r["db"]), P.bar(X, W, b, y, cw, 3))
    assert failed >= 1, mutation


def test_the_blobs_leave_no_row_undecided_at_the_reference_optimum():
    """The GPU test compares `predict` with the float64 argmax on the rows whose float64 top-two margin exceeds twice the logit bar
    and may leave out 1 % of them; on these seeded inputs no row is left out at the reference optimum (rounded to fp32, as the
    product keeps it)."""
    _paths()
    n, D, C, l2 = P.BLOBS["n"], P.BLOBS["D"], P.BLOBS["C"], P.BLOBS["l2"]
    X, y = P.blobs()
    theta = P.reference_solver(X, y, C, l2, gtol=1e-6)[0].reshape(C, D + 1)
    W, b = torch.from_numpy(theta[:, :D]).float(), torch.from_numpy(theta[:, D]).float()
    z = X.double() @ W.double().t() + b.double()
    top = z.topk(2, dim=1).values
    margin = top[:, 0] - top[:, 1]
    bar = P.logit_bar(X, W, b)
    print("smallest margin / (2 bar)", float((margin / (2 * bar)).min()))
    assert bool((margin > 2 * bar).all())
    accuracy = float((z.argmax(dim=1)[y >= 0] == y[y >= 0]).double().mean())
    assert 0.8 < accuracy < 1.0, accuracy                                         # the classes overlap: a real fit, not a separable toy


def test_support_table_and_partials_of_the_library():
    _paths()
    from mmgclip import _hip, head
    lib = _hip.load()
    for D in list(range(32, 1025, 32)) + [0, 16, 48, 1000, 1056, -32]:
        for C in (-1, 0, 1, 2, 3, 16, 31, 32, 33, 64):
            ok = lib.mmg_probe_rows_supported(D, C)
            assert ok == int(P.supported(D, C)) and head._HipProbeBackend.supported(D, C) == bool(ok), (D, C)
            for n, groups in ((1, 1), (33, 1), (33, 2), (33, 5), (1000, 3), (1000, 4096)):
                assert lib.mmg_probe_rows_partials_bytes(n, D, C, groups) == (P.partials_bytes(n, D, C, groups) if ok else 0), (D, C, n, groups)
    assert lib.mmg_probe_rows_partials_bytes(0, 64, 4, 1) == 0 and lib.mmg_probe_rows_partials_bytes(64, 64, 4, -1) == 0
    assert lib.mmg_probe_rows_partials_bytes(64, 64, 4, 4097) == 0
    assert lib.mmg_abi_version() == 5


def test_bad_arguments_are_rejected_without_a_gpu():
    """Validation comes before any HIP call, each message naming the limit."""
    _paths()
    import ctypes

    from mmgclip import _hip
    lib = _hip.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)

    def probe(X=p, W=p, b=p, labels=p, cw=None, n=1, D=32, C=2, groups=1, partials=p, out=p):
        return lib.mmg_probe_rows(X, W, b, labels, cw, n, D, C, groups, partials, out, None)
    for kw, msg in ((dict(n=0), b"n=0 must be positive"), (dict(n=-5), b"must be positive"),
                    (dict(D=100), b"multiple of 32 in [32,1024]"), (dict(D=0), b"multiple of 32 in [32,1024]"),
                    (dict(D=2048), b"multiple of 32 in [32,1024]"),
                    (dict(C=1), b"C=1 must be in [2,32]"), (dict(C=33), b"C=33 must be in [2,32]"), (dict(C=0), b"must be in [2,32]"),
                    (dict(groups=-1), b"n_groups=-1 must be in [0,4096]"), (dict(groups=5000), b"must be in [0,4096]"),
                    (dict(X=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(b=None), b"null pointer"),
                    (dict(labels=None), b"null pointer"), (dict(partials=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(partials=odd), b"8-byte aligned"), (dict(out=odd), b"8-byte aligned"), (dict(X=odd), b"16-byte aligned")):
        assert probe(**kw) != 0, kw
        assert msg in lib.mmg_last_error(), (kw, lib.mmg_last_error())
