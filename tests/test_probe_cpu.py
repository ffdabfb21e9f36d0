"""The linear probe, CPU side: `probe.LinearProbe` over gloo with world sizes 2 and 4, UNEVEN shards and one EMPTY shard (the device
arithmetic `head._HipProbeBackend` replaced, inside the worker processes only, by the fp32 emulation of tests/probe_ref.py; Comm,
LinearProbe and its L-BFGS are the product code): one evaluation inside the bar of the unsharded float64 reference, the fitted W, b
torch.equal across ranks and within the strong-convexity distance of the unsharded fit, `sweep` picking the same l2 everywhere; then
the probe's argument checks, the dense route against the emulation, `Evaluator.linear_probe`'s result keys and `evaluate_experiment`'s
results.txt with and without the new method."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import auroc_ref as A
from tests import probe_ref as P
from tests.test_averaged_fused_cpu import _free_port, _paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "mmg-clip_amd", "configs")
N, D, C, L2 = 210, 32, 3, 1e-2
L2S = (1.0, 1e-1, 1e-2)
NVAL = 90


def _rows_forward(x, y, scale, off, want):
    """`head.rows_forward` (the logit kernel `decision_function` takes on the device) in plain torch."""
    return None, None, (x @ y.t()) * scale


def _shards(total, world):
    """Uneven at both world sizes - [130, 80] and [112, 70, 28, 0] of 210 - and at world size 4 the last rank EMPTY."""
    if world == 2:
        return [total - 80, 80]
    c = [total // 2 + 7, total // 3, 0, 0]
    c[2] = total - c[0] - c[1]
    return c


def _problem():
    X, y = P.blobs(N + NVAL, D, C, seed=5)
    cw = None
    return X[:N].contiguous(), y[:N].contiguous(), X[N:].contiguous(), y[N:].clamp(min=0).contiguous(), cw


def _worker(rank, world, port, balanced, q):
    _paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from mmgclip import distributed, head, probe
    comm = distributed.init_from_env("gloo")
    head._HipProbeBackend = P.TorchProbeBackend                     # this worker process only
    head._HipAurocBackend = A.TorchAurocBackend
    head.rows_forward = _rows_forward
    probe.LinearProbe._use_fused = lambda self, X, C: True          # the emulation is "the kernel" here
    X, y, Xv, yv, _ = _problem()
    sc, vc = _shards(N, world), [NVAL // world + (r == 0) * (NVAL % world) for r in range(world)]
    s = slice(sum(sc[:rank]), sum(sc[:rank + 1]))
    v = slice(sum(vc[:rank]), sum(vc[:rank + 1]))
    Xl, yl = X[s].contiguous(), y[s].contiguous()
    lp = probe.LinearProbe(l2=L2, max_iter=300, gtol=1e-5, class_weight="balanced" if balanced else None, comm=comm)
    g = torch.Generator().manual_seed(1)
    W0, b0 = torch.randn(C, D, generator=g) * 0.2, torch.randn(C, generator=g) * 0.2
    one = lp.evaluate(Xl, yl, W0, b0)
    comm.report()
    lp.fit(Xl, yl, n_classes=C)
    calls = comm.report()
    # numpy arrays travel through the queue by value: a tensor travels as a handle to shared memory that dies with this process
    fitted = dict(weight=lp.weight.numpy().copy(), bias=lp.bias.numpy().copy(), n_iter=lp.n_iter_, converged=lp.converged_, grad=lp.grad_norm_,
                  objective=lp.objective_, n_eval=lp.n_evaluations_)
    sw = probe.LinearProbe(max_iter=100, gtol=1e-4, comm=comm).sweep(Xl, yl, Xv[v].contiguous(), yv[v].contiguous(), L2S, n_classes=C)
    q.put(dict(rank=rank, rows=sc[rank], one=one.numpy().copy(), calls=calls, fitted=fitted, sweep_l2=sw.l2, sweep=sw.sweep_,
               sweep_w=sw.weight.numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def _run(world, balanced):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, balanced, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in range(world)]
    for r in results:
        r["one"], r["sweep_w"] = torch.from_numpy(r["one"]), torch.from_numpy(r["sweep_w"])
        r["fitted"]["weight"], r["fitted"]["bias"] = torch.from_numpy(r["fitted"]["weight"]), torch.from_numpy(r["fitted"]["bias"])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return sorted(results, key=lambda r: r["rank"])


def _balanced_weights(y):
    counts = torch.bincount(y[y >= 0], minlength=C).double()
    return (counts.sum() / (C * counts)).float()


@pytest.mark.parametrize("balanced", [False, True])
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_fit_gloo(world, balanced):
    _paths()
    results = _run(world, balanced)
    X, y, Xv, yv, _ = _problem()
    cw = _balanced_weights(y) if balanced else None
    assert [r["rows"] for r in results] == _shards(N, world) and len({c for c in _shards(N, world) if c}) >= 2       # uneven, non-empty
    assert _shards(N, 2) == [130, 80] and _shards(N, 4) == [112, 70, 28, 0]                                            # and one empty
    # one evaluation at a fixed W: every rank holds the same all-reduced vector, inside the bar of the unsharded float64 reference
    g = torch.Generator().manual_seed(1)
    W0, b0 = torch.randn(C, D, generator=g) * 0.2, torch.randn(C, generator=g) * 0.2
    ref = P.reference(X, W0, b0, y)
    want = P.flat(ref["L"], ref["dW"], ref["db"])
    limit = P.bar(X, W0, b0, y, None, 1)                             # R = all rows in one accumulator: the widest of the groupings
    for r in results:
        assert torch.equal(r["one"], results[0]["one"])
        assert bool(((r["one"] - want).abs() <= limit).all()), float(((r["one"] - want).abs() / limit).max())
    # the fit: identical on every rank, converged, one all-reduce per evaluation (+ the label counts)
    f0 = results[0]["fitted"]
    for r in results:
        f = r["fitted"]
        assert torch.equal(f["weight"], f0["weight"]) and torch.equal(f["bias"], f0["bias"])
        assert (f["n_iter"], f["grad"], f["objective"]) == (f0["n_iter"], f0["grad"], f0["objective"])
        assert f["converged"] and f["grad"] <= 1e-5
        assert r["calls"]["all_reduce_calls"] == f["n_eval"] + 1 and r["calls"]["all_gather_calls"] == 0, r["calls"]
        assert r["calls"]["all_reduce_bytes"] == f["n_eval"] * (C * (D + 1) + 1) * 8 + C * 8
    # within the strong-convexity distance of the unsharded float64 fit
    theta_ref, _, g_ref, _, conv, _ = P.reference_solver(X, y, C, L2, cw, gtol=1e-9)
    assert conv
    theta = torch.cat([f0["weight"], f0["bias"][:, None]], dim=1).double().numpy().reshape(-1)
    g_dev = P.objective(theta, X, y, C, L2, cw)[1]
    dist_w = np.linalg.norm((theta - theta_ref).reshape(C, D + 1)[:, :D])
    bound = P.convexity_distance(g_dev, g_ref, L2)
    print("world", world, "balanced", balanced, "distance", dist_w, "bound", bound, "n_iter", f0["n_iter"])
    assert dist_w <= bound and bound < 0.1
    # sweep: the same l2, the same table, the same weights everywhere
    for r in results:
        assert r["sweep_l2"] == results[0]["sweep_l2"] and r["sweep"] == results[0]["sweep"] and torch.equal(r["sweep_w"], results[0]["sweep_w"])
    table = results[0]["sweep"]
    assert [t[0] for t in table] == sorted(L2S, reverse=True)
    best = max(t[1] for t in table)
    assert results[0]["sweep_l2"] == max(t[0] for t in table if t[1] == best)          # a tie goes to the larger l2


def test_unsharded_fit_sweep_and_state_dict(monkeypatch):
    _paths()
    from mmgclip import head, probe
    monkeypatch.setattr(head, "_HipProbeBackend", P.TorchProbeBackend)
    monkeypatch.setattr(head, "_HipAurocBackend", A.TorchAurocBackend)
    X, y, Xv, yv, _ = _problem()
    dense = probe.LinearProbe(l2=L2, max_iter=300, gtol=1e-5).fit(X, y)                  # on the CPU: the dense route, C from the labels
    assert dense.converged_ and dense.weight.shape == (C, D) and dense.classes.tolist() == [0, 1, 2] and dense.n_evaluations_ > dense.n_iter_
    monkeypatch.setattr(probe.LinearProbe, "_use_fused", lambda self, X, C: True)
    monkeypatch.setattr(head, "rows_forward", _rows_forward)
    fused = probe.LinearProbe(l2=L2, max_iter=300, gtol=1e-5).fit(X, y)
    g1 = P.objective(torch.cat([dense.weight, dense.bias[:, None]], 1).double().numpy().reshape(-1), X, y, C, L2)[1]
    g2 = P.objective(torch.cat([fused.weight, fused.bias[:, None]], 1).double().numpy().reshape(-1), X, y, C, L2)[1]
    assert float((dense.weight - fused.weight).double().norm()) <= P.convexity_distance(g1, g2, L2)
    z = fused.decision_function(Xv)
    assert torch.equal(z, Xv @ fused.weight.t() + fused.bias) and torch.equal(fused.predict(Xv), z.argmax(dim=1))
    assert torch.allclose(fused.predict_proba(Xv).sum(dim=1), torch.ones(NVAL))
    assert float((fused.predict(Xv) == yv).double().mean()) > 0.6
    state = fused.state_dict()
    assert set(state) == {"weight", "bias", "classes"}
    other = probe.LinearProbe().load_state_dict(state)
    assert torch.equal(other.predict(Xv), fused.predict(Xv))
    with pytest.raises(KeyError, match="classes"):
        probe.LinearProbe().load_state_dict({"weight": state["weight"], "bias": state["bias"]})
    with pytest.raises(RuntimeError, match="not fitted"):
        probe.LinearProbe().predict(Xv)
    # an l2 that is hit twice and a tie: constant validation labels make every AUROC nan, the first (largest) l2 stays
    sw = probe.LinearProbe(max_iter=30).sweep(X, y, Xv, torch.zeros(NVAL, dtype=torch.int64), [1e-2, 1.0, 1e-2], n_classes=C)
    assert sw.l2 == 1.0 and [t[0] for t in sw.sweep_] == [1.0, 1e-2]
    # max_iter = 0 keeps W0 = 0
    zero = probe.LinearProbe(max_iter=0).fit(X, y)
    assert not zero.converged_ and zero.n_iter_ == 0 and not bool(zero.weight.any()) and abs(zero.objective_ - np.log(3)) < 1e-6


def _macro_auc(p, y, C):
    from sklearn.metrics import roc_auc_score
    return float(np.mean([roc_auc_score(y == c, p[:, c]) for c in range(C)]))


def test_sweep_leaves_ignored_validation_rows_out_of_its_choice(monkeypatch):
    """45 of 60 validation rows carry the ignore label.  `ZeroShotAUROC` would count them as negatives of every class; on these
    seeded rows that changes the winner (sklearn's roc_auc_score on both readings, asserted here), so the l2 that `sweep` keeps
    tells which reading it took: the one without them."""
    _paths()
    from mmgclip import head, probe
    monkeypatch.setattr(head, "_HipAurocBackend", A.TorchAurocBackend)
    l2s = [1.0, 1e-1, 1e-2, 1e-3]
    X, y = P.blobs(150, 32, 3, seed=17)
    y = y.clamp(min=0)
    Xt, yt, Xv, yv = X[:90].contiguous(), y[:90].contiguous(), X[90:].contiguous(), y[90:].clone()
    yv[torch.arange(60) % 4 != 0] = -1
    known = (yv >= 0).numpy()
    assert known.sum() == 15 and set(yv[yv >= 0].tolist()) == {0, 1, 2}
    without, counted = [], []
    for l2 in l2s:
        p = probe.LinearProbe(l2=l2, max_iter=100).fit(Xt, yt, n_classes=3).predict_proba(Xv).numpy()
        without.append(_macro_auc(p[known], yv.numpy()[known], 3))
        counted.append(_macro_auc(p, yv.numpy(), 3))
    best_without = max(l for l, a in zip(l2s, without) if a == max(without))
    best_counted = max(l for l, a in zip(l2s, counted) if a == max(counted))
    assert best_without != best_counted, (without, counted)                   # the inputs can tell the two readings apart
    sw = probe.LinearProbe(max_iter=100).sweep(Xt, yt, Xv, yv, l2s, n_classes=3)
    assert sw.l2 == best_without and [t[0] for t in sw.sweep_] == l2s
    assert all(abs(t[1] - a) <= 1e-12 for t, a in zip(sw.sweep_, without)), (sw.sweep_, without)
    # y_val is checked like y
    with pytest.raises(ValueError, match=r"y_val must lie in \[-1, C\)"):
        probe.LinearProbe(max_iter=5).sweep(Xt, yt, Xv, yv - 1, l2s, n_classes=3)
    with pytest.raises(ValueError, match=r"y_val must lie in \[-1, C\)"):
        probe.LinearProbe(max_iter=5).sweep(Xt, yt, Xv, yv + 2, l2s)
    with pytest.raises(ValueError, match="y_val must be an int64 vector"):
        probe.LinearProbe(max_iter=5).sweep(Xt, yt, Xv, yv[:-1], l2s)
    with pytest.raises(ValueError, match="X_val has D=16"):
        probe.LinearProbe(max_iter=5).sweep(Xt, yt, Xv[:, :16].contiguous(), yv, l2s)


def test_dense_route_agrees_with_the_emulation_and_the_reference():
    _paths()
    from mmgclip import probe
    X, W, b, y, cw = P.random_case(257, 96, 3)
    ref = P.reference(X, W, b, y, cw)
    want = P.flat(ref["L"], ref["dW"], ref["db"])
    got = probe.LinearProbe.dense_evaluate(X, W, b, y, cw)
    assert got.dtype == torch.float64 and bool(((got - want).abs() <= P.bar(X, W, b, y, cw, 1)).all())
    got = probe.LinearProbe.dense_evaluate(X, W, b, y, None)
    ref = P.reference(X, W, b, y, None)
    assert bool(((got - P.flat(ref["L"], ref["dW"], ref["db"])).abs() <= P.bar(X, W, b, y, None, 1)).all())


def test_the_probe_rejects_what_it_cannot_fit():
    _paths()
    from mmgclip import probe
    X, y = P.blobs(40, 32, 3, seed=2)
    for kw, msg in ((dict(l2=0), "l2 must be"), (dict(l2=-1.0), "l2 must be"), (dict(max_iter=-1), "max_iter"), (dict(max_iter=2.5), "max_iter"),
                    (dict(gtol=0), "gtol"), (dict(class_weight="even"), "class_weight"), (dict(fused="yes"), "fused")):
        with pytest.raises(ValueError, match=msg):
            probe.LinearProbe(**kw)
    lp = probe.LinearProbe()
    with pytest.raises(ValueError, match="fp32"):
        lp.fit(X.double(), y)
    with pytest.raises(ValueError, match="contiguous"):
        lp.fit(X.t().contiguous().t(), y)
    with pytest.raises(ValueError, match=r"\[rows,D\]"):
        lp.fit(X[0], y)
    with pytest.raises(ValueError, match="int64"):
        lp.fit(X, y.int())
    with pytest.raises(ValueError, match="one label per row"):
        lp.fit(X, y[:-1])
    with pytest.raises(ValueError, match=r"\[-1, C\)"):
        lp.fit(X, y - 2)
    with pytest.raises(ValueError, match=r"\[-1, C\) with -1 the ignore label \(C=2\)"):
        lp.fit(X, y, n_classes=2)
    with pytest.raises(ValueError, match="at least two classes"):
        lp.fit(X, torch.zeros(40, dtype=torch.int64))
    with pytest.raises(ValueError, match="nothing to fit"):
        lp.fit(X, torch.full((40,), -1, dtype=torch.int64), n_classes=3)
    with pytest.raises(ValueError, match="C=3 finite non-negative"):
        probe.LinearProbe(class_weight=torch.ones(4)).fit(X, y)
    with pytest.raises(ValueError, match="fused=True needs a GPU tensor"):
        probe.LinearProbe(fused=True).fit(X, y)
    with pytest.raises(ValueError, match="l2s"):
        lp.sweep(X, y, X, y, [])
    fitted = probe.LinearProbe(max_iter=3).fit(X, y)
    with pytest.raises(ValueError, match="D=32"):
        fitted.predict(torch.zeros(2, 64))


# ---- Evaluator -----------------------------------------------------------------------------------------------------------------------
def _evaluator(monkeypatch, tmp_path=None, overrides=(), train=True):
    from mmgclip import evaluator, head
    from mmgclip.config import compose
    monkeypatch.setattr(head, "_HipAurocBackend", A.TorchAurocBackend)
    over = ["dataset.eval.method=[zeroshot_label_prompt]", "+dataset.eval.bootstrap_ci.ci=device", "+dataset.eval.bootstrap_ci.seed=3"]
    if tmp_path is not None:
        over.append(f"base.results_export_dir={tmp_path}")
    X, y = P.blobs(160, 32, 2, seed=9)
    y = y.clamp(min=0)
    labels = [{"BenignMalignantDatasetLabels": "malignant" if v else "benign"} for v in y.tolist()]
    batches = [dict(img=X[a:a + 32], prompt_labels=labels[a:a + 32]) for a in range(0, 160, 32)]
    ev = evaluator.Evaluator.__new__(evaluator.Evaluator)
    ev.config, ev.device = compose(CFG_DIR, "train_binary_class_clf", over + list(overrides)), torch.device("cpu")
    ev.model = torch.nn.Identity()
    ev.test_dataloader, ev.train_dataloader = batches[3:], batches[:3] if train else None
    ev.tokenizer = None
    ev.encode_image = lambda batch, as_numpy=True: batch["img"]
    g = np.random.default_rng(4)
    ev.prompt_similarities = lambda emb, prompts, use_logits=True: g.standard_normal((len(emb), len(prompts))).astype(np.float32)
    return ev, X, y, labels


def test_evaluator_linear_probe_result_keys(monkeypatch):
    _paths()
    from mmgclip import evaluator
    ev, X, y, labels = _evaluator(monkeypatch)
    classes = dict(evaluator.ENUMS["BenignMalignantDatasetLabels"])
    res = ev.linear_probe(X[:96], labels[:96], X[96:], labels[96:], classes, "BenignMalignantDatasetLabels", n_iterations=40, seed=3, l2=1e-2)
    assert list(res) == ["accuracy", "confusion_matrix", "auc", "auc_ci_mean", "auc_ci_lower", "auc_ci_higher", "l2", "n_iter", "converged"]
    assert list(res["auc"]) == ["benign", "malignant"] and abs(res["auc"]["benign"] - res["auc"]["malignant"]) < 0.01
    cm = res["confusion_matrix"]
    assert isinstance(cm, list) and len(cm) == 2 and all(isinstance(r, list) and len(r) == 2 for r in cm) and sum(map(sum, cm)) == 64
    assert res["accuracy"] == (cm[0][0] + cm[1][1]) / 64 and res["accuracy"] > 0.6 and res["auc"]["malignant"] > 0.6
    assert res["auc_ci_lower"] <= res["auc_ci_mean"] <= res["auc_ci_higher"] and res["l2"] == 1e-2 and res["converged"]
    assert res == ev.linear_probe(X[:96], labels[:96], X[96:], labels[96:], classes, "BenignMalignantDatasetLabels", n_iterations=40, seed=3, l2=1e-2)
    plain = ev.linear_probe(X[:96], labels[:96], X[96:], labels[96:], classes, "BenignMalignantDatasetLabels", ci=None, l2s=[1.0, 1e-2], max_iter=50)
    assert list(plain) == ["accuracy", "confusion_matrix", "auc", "l2", "n_iter", "converged"] and plain["l2"] in (1.0, 1e-2)
    # `unknown` is left out: of the classes, of the fit (ignored rows) and of the test figures
    shapes = dict(evaluator.ENUMS["MassShapeLabels"])
    names = ["unknown", "oval", "round", "irregular"]
    sl = [{"MassShapeLabels": names[(i % 3) + 1] if i % 5 else "unknown"} for i in range(160)]
    Xs = X + torch.nn.functional.one_hot(torch.arange(160) % 3, 32).float() * 3
    res = ev.linear_probe(Xs[:96], sl[:96], Xs[96:], sl[96:], shapes, "MassShapeLabels", l2=1e-2)
    assert list(res["auc"]) == ["oval", "round", "irregular"] and len(res["confusion_matrix"]) == 3 and "auc_ci_mean" not in res
    assert sum(map(sum, res["confusion_matrix"])) == sum(1 for d in sl[96:] if d["MassShapeLabels"] != "unknown") and res["accuracy"] > 0.7
    with pytest.raises(ValueError, match="ci must be"):
        ev.linear_probe(X[:96], labels[:96], X[96:], labels[96:], classes, "BenignMalignantDatasetLabels", ci="host")
    # a name that is neither a class nor `unknown` is an error, in the train and in the test labels alike
    for bad in (sl[:5] + [{"MassShapeLabels": "ovall"}] + sl[6:96], sl[96:]), (sl[:96], sl[96:-1] + [{"MassShapeLabels": "lobulated"}]):
        with pytest.raises(KeyError, match="ovall|lobulated"):
            ev.linear_probe(Xs[:96], bad[0], Xs[96:], bad[1], shapes, "MassShapeLabels", l2=1e-2)
    # the l2s path: held-out train rows labelled `unknown` never reach the AUROC
    from mmgclip import zeroshot_auroc
    seen = []
    update = zeroshot_auroc.ZeroShotAUROC.update

    def spy(self, name, scores, targets, class_values):
        seen.append((name, torch.as_tensor(targets).clone()))
        return update(self, name, scores, targets, class_values)
    monkeypatch.setattr(zeroshot_auroc.ZeroShotAUROC, "update", spy)
    sl2 = [{"MassShapeLabels": "unknown" if i % 10 == 4 else names[(i % 3) + 1]} for i in range(160)]       # half of the held-out rows
    assert sum(1 for i in range(96) if i % 5 == 4 and sl2[i]["MassShapeLabels"] == "unknown") == 10
    res = ev.linear_probe(Xs[:96], sl2[:96], Xs[96:], sl2[96:], shapes, "MassShapeLabels", l2s=[1.0, 1e-2], max_iter=50)
    val = [t for name, t in seen if name == "val"]
    assert all(t.numel() == 9 for t in val)                             # 19 held-out rows, 10 of them `unknown`
    assert len(val) == 2 and all(bool((t >= 0).all()) for _, t in seen) and res["l2"] in (1.0, 1e-2)


def test_evaluate_experiment_results_file_with_and_without_the_probe(monkeypatch, tmp_path):
    _paths()
    from mmgclip import evaluator
    from mmgclip.utils.logger import logger
    key = "BenignMalignantDatasetLabels"
    classes = dict(evaluator.ENUMS[key])

    def text(results):
        return "".join(str(r) + "\n\n" for r in results)
    # without the new method: what zeroshot_label_prompt alone gives, byte for byte, and no train batch is touched
    ev, X, y, labels = _evaluator(monkeypatch, tmp_path / "a")
    ev.train_dataloader = iter(())                                      # would be exhausted if read; it is not even asked
    before = ev.evaluate_experiment()
    ev2, *_ = _evaluator(monkeypatch)
    want = ev2.zeroshot_label_prompt(image_embeddings=X[96:], label_names=labels[96:], classes_dict=classes, key=key, ci="device", seed=3)
    assert before == [want] and open(tmp_path / "a" / "results.txt").read() == text([want])
    # with it: the same first entry, then the probe's
    over = ["dataset.eval.method=[zeroshot_label_prompt,linear_probe]", "+dataset.eval.linear_probe.l2=0.01", "+dataset.eval.linear_probe.max_iter=60"]
    ev, *_ = _evaluator(monkeypatch, tmp_path / "b", over)
    assert ev.linear_probe_config() == {"l2": 0.01, "max_iter": 60}
    both = ev.evaluate_experiment()
    assert both[0] == want and len(both) == 2 and both[1]["l2"] == 0.01 and "confusion_matrix" in both[1]
    assert both[1] == ev.linear_probe(X[:96], labels[:96], X[96:], labels[96:], classes, key, l2=0.01, max_iter=60)
    assert open(tmp_path / "b" / "results.txt").read() == text(both)
    # without a train dataloader: logged and skipped, the file as before
    warned = []
    monkeypatch.setattr(logger, "warning", lambda msg, *a, **k: warned.append(str(msg)))
    ev, *_ = _evaluator(monkeypatch, tmp_path / "c", over, train=False)
    assert ev.evaluate_experiment() == [want] and open(tmp_path / "c" / "results.txt").read() == text([want])
    assert len(warned) == 1 and "linear_probe" in warned[0] and "skipped" in warned[0]
    ev, *_ = _evaluator(monkeypatch, None, ["+dataset.eval.linear_probe.l2=0.1", "+dataset.eval.linear_probe.l2s=[1.0]"])
    with pytest.raises(ValueError, match="not both"):
        ev.linear_probe_config()
    ev, *_ = _evaluator(monkeypatch, None, ["+dataset.eval.linear_probe.lr=0.1"])
    with pytest.raises(ValueError, match="unknown keys"):
        ev.linear_probe_config()
    import inspect
    assert inspect.signature(evaluator.Evaluator.__init__).parameters["train_dataloader"].default is None
