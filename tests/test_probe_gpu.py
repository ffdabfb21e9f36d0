"""The linear probe on the MI355X: the kernel of csrc/probe_head.hip through `_hip.call` on the test's own buffers, then
`head._HipProbeBackend`, `probe.LinearProbe` and the dense route, against the float64 reference of tests/probe_ref.py.

Every kernel call writes into an `out` pre-filled with NaN and followed by 32 sentinel doubles, and into a `partials` buffer of exactly
mmg_probe_rows_partials_bytes followed by 32 sentinel doubles: no output may keep its fill and no sentinel may change.

Exact regime (torch.equal against int64 arithmetic; integer X in [-8,8]): W = 0 with C in {2, 4, 32}, where p = 1/C and dW, db are exact
multiples of 1/C (the row-to-label, class-to-row and column maps and the padding of 30 / 28 / 0 classes), and saturated integer logits,
where p is exactly one-hot and L an exact integer (the bias add and the label pick); ignore labels and power-of-two class weights in
both; n in {1, 31, 32, 33, 200} x n_groups in {1, 2, 3, 0}, all n_groups the same bits.
Random regime: the shapes of probe_ref.RANDOM_SHAPES within the derived bar `probe_ref.bar`."""
import numpy as np
import pytest
import torch

from tests import probe_ref as P

pytestmark = pytest.mark.gpu
TAIL = 32
SENTINEL = 12345.0


def _launch(dev, X, W, b, y, cw, n_groups):
    """One call of mmg_probe_rows -> float64 [C (D+1) + 1] on the CPU; fresh, poisoned, fenced buffers."""
    from mmgclip import _hip
    from mmgclip._hip import call, ptr, stream
    n, D = X.shape
    C = W.shape[0]
    E = C * (D + 1) + 1
    nbytes = _hip.load().mmg_probe_rows_partials_bytes(n, D, C, n_groups)
    assert nbytes > 0 and nbytes % 8 == 0
    Xd, Wd, bd, yd = X.to(dev).contiguous(), W.to(dev).contiguous(), b.to(dev).contiguous(), y.to(dev).contiguous()
    cd = None if cw is None else cw.to(dev).contiguous()
    out = torch.full((E + TAIL,), SENTINEL, device=dev, dtype=torch.float64)
    out[:E] = float("nan")
    partials = torch.full((nbytes // 8 + TAIL,), SENTINEL, device=dev, dtype=torch.float64)
    call("mmg_probe_rows", ptr(Xd), ptr(Wd), ptr(bd), ptr(yd), ptr(cd), n, D, C, n_groups, ptr(partials), ptr(out), stream())
    torch.cuda.synchronize()
    assert bool((out[E:] == SENTINEL).all()) and bool((partials[nbytes // 8:] == SENTINEL).all()), "a sentinel after a buffer changed"
    res = out[:E].cpu()
    assert not bool(torch.isnan(res).any()), "an output kept its NaN fill (or the kernel produced one)"
    return res


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [2, 4, 32])
def test_zero_weights_give_exact_multiples_of_one_over_c(dev, C, weighted):
    D = 64
    for n in P.EXACT_NS:
        X, W, b, y, cw, dW, db = P.zero_weight_case(n, D, C, weighted)
        r = P.reference(X, W, b, y, cw)
        want = P.flat(r["L"], dW, db)
        losses = []
        for groups in P.EXACT_GROUPS:
            got = _launch(dev, X, W, b, y, cw, groups)
            assert torch.equal(got[:-1], want[:-1]), (n, groups, torch.nonzero(got[:-1] != want[:-1]).flatten()[:8].tolist())
            assert abs(float(got[-1] - want[-1])) <= float(P.bar(X, W, b, y, cw, groups)[-1]), (n, groups)      # L = S ln C is not exact
            losses.append(got[-1])
        # .. but the same bits for every n_groups: the row losses are the fp32 ln C times a power of two, and an fp64 sum of a few
        # hundred of them is exact in any order
        assert all(torch.equal(v, losses[0]) for v in losses), (n, [float(v) for v in losses])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", [(64, 2), (64, 4), (32, 32), (160, 5)])
def test_saturated_integer_logits_are_exactly_one_hot(dev, shape, weighted):
    D, C = shape
    for n in P.EXACT_NS:
        X, W, b, y, cw, dW, db, L = P.saturated_case(n, D, C, weighted)
        want = P.flat(L, dW, db)
        for groups in P.EXACT_GROUPS:
            got = _launch(dev, X, W, b, y, cw, groups)
            assert torch.equal(got, want), (n, groups, torch.nonzero(got != want).flatten()[:8].tolist())


@pytest.mark.parametrize("shape", P.RANDOM_SHAPES)
def test_random_rows_inside_the_bar(dev, shape):
    n, D, C = shape
    X, W, b, y, cw = P.random_case(n, D, C)
    r = P.reference(X, W, b, y, cw)
    want = P.flat(r["L"], r["dW"], r["db"])
    for groups, weights in ((0, cw), (3, cw), (0, None)):
        if weights is None:
            r = P.reference(X, W, b, y, None)
            want = P.flat(r["L"], r["dW"], r["db"])
        got = _launch(dev, X, W, b, y, weights, groups)
        limit = P.bar(X, W, b, y, weights, groups, auto=torch.cuda.get_device_properties(dev).multi_processor_count)
        ratio = float(((got - want).abs() / limit).max())
        print(shape, "groups", groups, "weighted", weights is not None, "worst |error| / bar", ratio)
        assert ratio <= 1.0
        again = _launch(dev, X, W, b, y, weights, groups)
        assert torch.equal(got, again)                                   # two launches on the same inputs: the same bits


def test_backend_route_and_dense_route_agree(dev):
    """The backend's own buffers; the dense torch route inside the same bar; an unsupported (D, C) falls back to the dense route;
    fused=True on it is refused."""
    from mmgclip import head, probe
    X, W, b, y, cw = P.random_case(257, 96, 3)
    r = P.reference(X, W, b, y, cw)
    want = P.flat(r["L"], r["dW"], r["db"])
    Xd, Wd, bd, yd, cd = (t.to(dev) for t in (X, W, b, y, cw))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    limit = P.bar(X, W, b, y, cw, 0, auto=cus)
    fused = head._HipProbeBackend.evaluate(Xd, Wd, bd, yd, cd)
    dense = probe.LinearProbe.dense_evaluate(Xd, Wd, bd, yd, cd)
    assert fused.is_cuda and fused.dtype == torch.float64 and dense.dtype == torch.float64
    assert bool(((fused.cpu() - want).abs() <= limit).all()) and bool(((dense.cpu() - want).abs() <= P.bar(X, W, b, y, cw, 1)).all())
    lp = probe.LinearProbe()
    assert torch.equal(lp.evaluate(Xd, yd, Wd, bd, cd), fused)
    assert torch.equal(probe.LinearProbe(fused=False).evaluate(Xd, yd, Wd, bd, cd), dense)
    # D = 48 is no multiple of 32, C = 40 is above 32: the dense route, silently for fused=None, refused for fused=True
    for n, D, C in ((100, 48, 3), (100, 64, 40)):
        X2, W2, b2, y2, cw2 = P.random_case(n, D, C, seed=1)
        assert not head._HipProbeBackend.supported(D, C)
        X2d, W2d, b2d, y2d = X2.to(dev), W2.to(dev), b2.to(dev), y2.to(dev)
        got = probe.LinearProbe().evaluate(X2d, y2d, W2d, b2d)
        assert torch.equal(got, probe.LinearProbe.dense_evaluate(X2d, W2d, b2d, y2d))
        r2 = P.reference(X2, W2, b2, y2)
        assert bool(((got.cpu() - P.flat(r2["L"], r2["dW"], r2["db"])).abs() <= P.bar(X2, W2, b2, y2, None, 1)).all())
        with pytest.raises(ValueError, match="fused=True needs"):
            probe.LinearProbe(fused=True).evaluate(X2d, y2d, W2d, b2d)
        with pytest.raises(ValueError, match=r"D % 32 == 0 in \[32,1024\], 2 <= C <= 32"):
            head._HipProbeBackend.evaluate(X2d, W2d, b2d, y2d)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        _launch_raw_bad(dev)


def _launch_raw_bad(dev):
    from mmgclip._hip import call, ptr, stream
    t = torch.zeros(64, device=dev, dtype=torch.float64)
    call("mmg_probe_rows", ptr(t), ptr(t), ptr(t), ptr(t), None, 1, 48, 2, 1, ptr(t), ptr(t), stream())


def test_fit_on_blobs_converges_and_predicts(dev):
    """n = 600, D = 64, C = 3, l2 = 1e-2: the fit converges; the float64 gradient at the device's solution is at most gtol plus the
    bar; decision_function within the logit bar of float64 at the device's own W; predict = the float64 argmax on every row whose
    float64 top-two margin exceeds twice that bar, at most 1 % of the rows left out (the CPU reference test: none at the reference
    optimum); the fused and the dense fit within the strong-convexity distance of each other and of the float64 optimum."""
    from mmgclip import probe
    n, D, C, l2 = P.BLOBS["n"], P.BLOBS["D"], P.BLOBS["C"], P.BLOBS["l2"]
    gtol = 1e-4
    X, y = P.blobs()
    Xd, yd = X.to(dev), y.to(dev)
    lp = probe.LinearProbe(l2=l2, max_iter=200, gtol=gtol).fit(Xd, yd)
    assert lp.converged_ and lp.grad_norm_ <= gtol and 0 < lp.n_iter_ < 200 and lp.weight.is_cuda and lp.weight.shape == (C, D)
    W, b = lp.weight.cpu(), lp.bias.cpu()
    theta = torch.cat([W, b[:, None]], dim=1).double().numpy().reshape(-1)
    F, g = P.objective(theta, X, y, C, l2)
    S = P.weight_sum(y)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    gbar = (P.bar(X, W, b, y, None, 0, auto=cus)[:-1] / S).numpy()
    print("n_iter", lp.n_iter_, "evaluations", lp.n_evaluations_, "max |g64|", np.abs(g).max(), "worst bar", gbar.max(), "F", F, lp.objective_)
    assert bool((np.abs(g) <= gtol + gbar).all())
    # prediction
    z64 = X.double() @ W.double().t() + b.double()
    zbar = P.logit_bar(X, W, b)
    z = lp.decision_function(Xd)
    assert z.is_cuda and z.dtype == torch.float32 and bool(((z.cpu().double() - z64).abs() <= zbar[:, None]).all())
    top = z64.topk(2, dim=1).values
    decided = (top[:, 0] - top[:, 1]) > 2 * zbar
    assert int((~decided).sum()) <= n // 100
    pred = lp.predict(Xd)
    assert pred.dtype == torch.int64 and torch.equal(pred.cpu()[decided], z64.argmax(dim=1)[decided])
    proba = lp.predict_proba(Xd)
    assert bool(((proba.sum(dim=1) - 1).abs() < 1e-5).all()) and torch.equal(proba.argmax(dim=1), z.argmax(dim=1))
    # against the dense route and the float64 optimum
    dense = probe.LinearProbe(l2=l2, max_iter=200, gtol=gtol, fused=False).fit(Xd, yd)
    g_dense = P.objective(torch.cat([dense.weight.cpu(), dense.bias.cpu()[:, None]], 1).double().numpy().reshape(-1), X, y, C, l2)[1]
    theta_ref, _, g_ref, _, conv, _ = P.reference_solver(X, y, C, l2, gtol=1e-9)
    assert conv and dense.converged_
    assert float((dense.weight.cpu() - W).double().norm()) <= P.convexity_distance(g, g_dense, l2)
    assert np.linalg.norm((theta - theta_ref).reshape(C, D + 1)[:, :D]) <= P.convexity_distance(g, g_ref, l2)
    # balanced weights and a sweep run on the device too
    bal = probe.LinearProbe(l2=l2, class_weight="balanced").fit(Xd, yd)
    assert bal.converged_
    sw = probe.LinearProbe(max_iter=100).sweep(Xd[:480].contiguous(), yd[:480].contiguous(), Xd[480:].contiguous(),
                                               yd[480:].clamp(min=0).contiguous(), [1.0, 1e-2])
    assert sw.l2 in (1.0, 1e-2) and len(sw.sweep_) == 2 and all(0.5 < t[1] <= 1.0 for t in sw.sweep_)


def test_evaluator_linear_probe_on_the_device(dev):
    """`Evaluator.linear_probe` end to end on the device: the probe kernel, the logit kernel and the AUROC kernels."""
    from mmgclip import evaluator
    X, y = P.blobs(320, 64, 2, seed=9)
    y = y.clamp(min=0)
    labels = [{"HasMassLabels": "mass" if v else "nomass"} for v in y.tolist()]
    ev = evaluator.Evaluator.__new__(evaluator.Evaluator)
    ev.device = dev
    res = ev.linear_probe(X[:200], labels[:200], X[200:], labels[200:], dict(evaluator.ENUMS["HasMassLabels"]), "HasMassLabels",
                          n_iterations=50, seed=1, l2=1e-2)
    assert list(res) == ["accuracy", "confusion_matrix", "auc", "auc_ci_mean", "auc_ci_lower", "auc_ci_higher", "l2", "n_iter", "converged"]
    assert res["converged"] and res["accuracy"] > 0.7 and res["auc"]["mass"] > 0.8 and sum(map(sum, res["confusion_matrix"])) == 120
    assert res["auc_ci_lower"] <= res["auc"]["mass"] <= res["auc_ci_higher"]
