"""The zero-shot AUROC, CPU side: `zeroshot_auroc.ZeroShotAUROC` over gloo with world sizes 2 and 4 and UNEVEN shards (the device
arithmetic `head._HipAurocBackend` replaced, inside the worker processes only, by the torch int64 emulation of tests/auroc_ref.py; Comm
and ZeroShotAUROC are the product code), chunked replicates, the config surface and its wiring into `ClassifierExperiment.validate()`,
the Evaluator's `ci` switch and the library's argument checks.  Integers in, correctly rounded divisions out: every comparison is `==`."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import auroc_ref as A
from tests.test_averaged_fused_cpu import _free_port, _paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "mmg-clip_amd", "configs")
N, BOOT, SEED = 75, 48, 5


def _shards(world):
    """Uneven on purpose: [39, 36] and [27, 17, 16, 15] of the 75."""
    c = [N // world - r for r in range(world)]
    c[0] += N - sum(c)
    return c


def _tasks():
    """75 samples; the 4-class task's class 3 lives in the first 20 samples only, so the later shards hold no positive of it."""
    tasks = A.example_tasks(N, seed=9)
    shapes, t4, values = tasks["shapes"]
    t4 = t4.copy()
    t4[20:][t4[20:] == 3] = 2
    t4[:3] = 3
    tasks["shapes"] = (shapes, t4, values)
    return tasks


def _feed(z, tasks, sl, batch):
    for name, (scores, targets, values) in tasks.items():
        s, t = torch.from_numpy(scores[sl]), torch.from_numpy(targets[sl])
        for a in range(0, s.shape[0], batch):
            z.update(name, s[a:a + batch], t[a:a + batch], values)


def _worker(rank, world, port, q):
    _paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from mmgclip import distributed, head, zeroshot_auroc
    comm = distributed.init_from_env("gloo")
    counts = _shards(world)
    head._HipAurocBackend = A.TorchAurocBackend                  # this worker process only
    z = zeroshot_auroc.ZeroShotAUROC(n_bootstrap=BOOT, seed=SEED, comm=comm)
    _feed(z, _tasks(), slice(sum(counts[:rank]), sum(counts[:rank + 1])), 16)
    out = z.compute()
    q.put(dict(rank=rank, result=out, calls=comm.report()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_dict_equals_the_unsharded_reference_gloo(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    tasks = _tasks()
    want = A.reference({k: v for k, v in tasks.items()}, BOOT, SEED)
    t4 = tasks["shapes"][1]
    counts = _shards(world)
    assert (t4[counts[0]:] != 3).all() and (t4 == 3).sum() >= 3, "the later shards must hold no positive of class 3"
    assert want["shapes"]["n_classes"] == 4 and want["malig"]["n_valid"] == BOOT and 0.5 < want["malig"]["auc"] < 1.0
    assert want["malig"]["ci_lower"] < want["malig"]["auc"] < want["malig"]["ci_upper"]
    for r in results:
        assert r["result"] == want, (r["rank"], r["result"], want)
        c = r["calls"]          # per task the shard sizes, the scores and the targets; ONE all-reduce of every task's U2
        assert c["all_gather_calls"] == 6 and c["all_reduce_calls"] == 1, c
        assert c["all_reduce_bytes"] == (1 + 4) * (1 + BOOT) * 8, c


def _compute(tasks, monkeypatch, batch=64, **kw):
    _paths()
    from mmgclip import head, zeroshot_auroc
    monkeypatch.setattr(head, "_HipAurocBackend", A.TorchAurocBackend)
    z = zeroshot_auroc.ZeroShotAUROC(**kw)
    _feed(z, tasks, slice(None), batch)
    return z.compute()


def test_unsharded_in_batches_equals_the_reference_and_chunking_does_not_matter(monkeypatch):
    tasks = A.example_tasks(150)
    want = A.reference(tasks, 64, SEED)
    got = _compute(tasks, monkeypatch, n_bootstrap=64, seed=SEED)                       # 64 / 64 / 22
    assert got == want
    assert list(got) == ["malig", "shapes"] and list(got["shapes"]["classes"]) == [0, 1, 2, 3]
    assert set(got["malig"]) == {"auc", "n_classes", "ci_mean", "ci_lower", "ci_upper", "n_valid", "classes"}
    assert got["malig"]["auc"] == got["malig"]["classes"][1]["auc"] and got["malig"]["ci_mean"] == got["malig"]["classes"][1]["ci_mean"]
    # 150 samples pad to 160 columns: 4 * 160 + 32 = 672 bytes per replicate, so 7 replicates per chunk, then 1
    from mmgclip.zeroshot_auroc import replicates_per_chunk
    assert [replicates_per_chunk(150, cap) for cap in (7 * 672, 7 * 672 - 1, 672, 1, 64 << 20)] == [7, 6, 1, 1, 65535]
    for cap in (7 * 672, 672, 1):
        assert _compute(tasks, monkeypatch, n_bootstrap=64, seed=SEED, max_weight_bytes=cap) == want
    assert _compute(tasks, monkeypatch, n_bootstrap=64, seed=SEED + 1)["malig"]["ci_lower"] != want["malig"]["ci_lower"]
    point = _compute(tasks, monkeypatch, n_bootstrap=0, seed=SEED)
    assert point == A.reference(tasks, 0, SEED) and set(point["malig"]) == {"auc", "n_classes", "classes"}


def test_a_class_without_positives_or_negatives_is_nan_and_launches_nothing(monkeypatch):
    _paths()
    from mmgclip import head, zeroshot_auroc
    calls = []

    class Spy(A.TorchAurocBackend):
        @staticmethod
        def pairs(s_pos, s_neg, w_pos, w_neg, neg_total=None):
            calls.append((s_pos.shape[0], s_neg.shape[0]))
            return A.TorchAurocBackend.pairs(s_pos, s_neg, w_pos, w_neg, neg_total)
    monkeypatch.setattr(head, "_HipAurocBackend", Spy)
    g = np.random.default_rng(0)
    scores = g.standard_normal((40, 3)).astype(np.float32)
    targets = np.array([0] * 30 + [1] * 10, dtype=np.int64)                 # class 2 has no positive
    tasks = {"t": (scores, targets, [0, 1, 2]), "all": (scores[:, :1], np.ones(40, dtype=np.int64), [1])}      # `all`: no negative
    z = zeroshot_auroc.ZeroShotAUROC(n_bootstrap=8, seed=SEED)
    _feed(z, tasks, slice(None), 64)
    got = z.compute()
    assert A.same(got, A.reference(tasks, 8, SEED))
    assert math.isnan(got["t"]["classes"][2]["auc"]) and got["t"]["classes"][2]["n_pos"] == 0 and got["t"]["classes"][2]["n_valid"] == 0
    assert got["t"]["n_classes"] == 2 and not math.isnan(got["t"]["auc"])
    assert math.isnan(got["all"]["auc"]) and got["all"]["n_classes"] == 0 and got["all"]["classes"][1]["n_neg"] == 0
    assert sorted(set(calls)) == [(10, 30), (30, 10)], calls
    with pytest.raises(ValueError, match="before any update"):
        zeroshot_auroc.ZeroShotAUROC().compute()
    with pytest.raises(ValueError, match="class values"):
        z.update("t", torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), [0, 1])


def test_config_fields_are_parsed_and_bad_ones_rejected():
    _paths()
    from mmgclip import zeroshot_auroc
    from mmgclip.config import compose
    cfg = compose(CFG_DIR, "train_binary_class_clf", [])
    assert "zeroshot_auroc" not in cfg.experiments.config and zeroshot_auroc.parse_config(None) is None
    for name in ("train_binary_class_clf", "train_prompt_clf"):
        cfg = compose(CFG_DIR, name, ["+experiments/config/zeroshot_auroc=bootstrap"])
        node = cfg.experiments.config.zeroshot_auroc
        assert (node.n_bootstrap, node.seed) == (1000, 0)
        assert cfg.experiments.config.experiment_name and "metrics" in cfg.experiments.config
        assert zeroshot_auroc.parse_config(node) == dict(n_bootstrap=1000, seed=0)
    cfg = compose(CFG_DIR, "train_binary_class_clf", ["+experiments/config/zeroshot_auroc=bootstrap",
                                                      "experiments.config.zeroshot_auroc.n_bootstrap=200", "experiments.config.zeroshot_auroc.seed=7"])
    z = zeroshot_auroc.ZeroShotAUROC(**zeroshot_auroc.parse_config(cfg.experiments.config.zeroshot_auroc))
    assert (z.n_bootstrap, z.seed, z.comm, z.max_weight_bytes) == (200, 7, None, 64 << 20)
    assert zeroshot_auroc.parse_config({"seed": 3}) == {"seed": 3}
    for bad in (-1, 1.5, "10", True, [1000]):
        with pytest.raises(ValueError, match="n_bootstrap"):
            zeroshot_auroc.parse_config({"n_bootstrap": bad})
    for bad in (-1, 0.5, "0", 2 ** 64):
        with pytest.raises(ValueError, match="seed"):
            zeroshot_auroc.parse_config({"seed": bad})
    with pytest.raises(ValueError, match="unknown keys"):
        zeroshot_auroc.parse_config({"n_boot": 10})
    with pytest.raises(ValueError, match="mapping"):
        zeroshot_auroc.parse_config(1000)
    with pytest.raises(ValueError, match="max_weight_bytes"):
        zeroshot_auroc.ZeroShotAUROC(max_weight_bytes=0)


# ---- validate() -------------------------------------------------------------------------------------------------------------------------
class _TinyPrompts(torch.nn.Module):
    """validate()'s loop without towers: the batch's image embeddings come back as they are, a prompt's embedding is a fixed
    function of its token ids."""

    def __init__(self, config=None):
        super().__init__()
        self.text_encoder = torch.nn.Linear(16, 8, bias=False)
        self.text_encoder.config = type("C", (), {"vocab_size": 3000})()
        self.text_projection_layer = None
        self.logit_scale = torch.nn.Parameter(torch.tensor(0.0))

    def count_parameters(self, model):
        return 0

    def encode_text(self, batch, **kw):
        ids = batch["text_tokens"]["input_ids"].double()
        k = ids.shape[0]
        g = torch.Generator().manual_seed(int(ids.sum()) % 1000)
        return torch.randn(k, 32, generator=g)

    def forward(self, batch, **kw):
        return {"image_embeddings": batch["img"], "text_embeddings": batch["img"], "logit_scale": self.logit_scale.exp()}


class _Scalars:
    def __init__(self):
        self.seen = {}

    def add_scalar(self, name, value, step):
        self.seen[name] = (value, step)


def _rows_forward(x, y, scale, off, want):
    return None, None, (x.float() @ y.float().t()) * scale


def _experiment(tmp_path, monkeypatch, extra):
    from mmgclip import head
    from mmgclip.config import compose
    from mmgclip.experiments import ClassifierExperiment as CE
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(CE, "model", _TinyPrompts)
    monkeypatch.setattr(head, "rows_forward", _rows_forward)
    monkeypatch.setattr(head.L2Normalize, "apply", staticmethod(lambda t: torch.nn.functional.normalize(t, dim=1)))
    over = [f"checkpoints.checkpoints_export_dir={tmp_path}", f"base.tensorboard_export_dir={tmp_path}", "experiments.config.metrics=[BenignMalignantDatasetLabels,MassShapeLabels,birads]"]
    g = torch.Generator().manual_seed(2)
    img = torch.nn.functional.normalize(torch.randn(70, 32, generator=g), dim=1)
    malig = torch.randint(0, 2, (70,), generator=g).tolist()
    shape = torch.randint(0, 4, (70,), generator=g).tolist()
    birads = [("unknown", 0, 1, 2, 3, 4, 5, 6)[v] for v in torch.randint(0, 8, (70,), generator=g).tolist()]
    labels = [{"BenignMalignantDatasetLabels": m, "MassShapeLabels": s, "BIRADS": b} for m, s, b in zip(malig, shape, birads)]
    loader = [dict(img=img[a:a + 32], prompt_labels=labels[a:a + 32]) for a in range(0, 70, 32)]
    exp = CE.ClassifierExperiment(config=compose(CFG_DIR, "train_binary_class_clf", over + list(extra)), train_dataloader=[],
                                  valid_dataloader=loader)
    exp.criterion = lambda **out: (out["image_embeddings"].sum() * 0 + 1.5, None)
    exp.writer = _Scalars()
    return exp


def test_validate_without_the_key_builds_no_zeroshot_auroc(tmp_path, monkeypatch):
    _paths()
    from mmgclip import zeroshot_auroc

    class Forbidden:
        def __init__(self, *a, **k):
            raise AssertionError("validate() built a ZeroShotAUROC although experiments.config.zeroshot_auroc is absent")
    monkeypatch.setattr(zeroshot_auroc, "ZeroShotAUROC", Forbidden)
    seen = []
    for extra in ([], ["+experiments.config.zeroshot_auroc=null"]):
        exp = _experiment(tmp_path, monkeypatch, extra)
        seen.append(exp.validate())
        assert exp.zeroshot is None and set(exp.writer.seen) == {"loss/val", "auc/val/malig", "auc/val/shapes", "auc/val/birads", "auc/val/average"}
    assert seen[0] == seen[1] and seen[0][0] == 1.5 and all(0.0 < v < 1.0 for v in seen[0][1:])


def test_validate_with_the_key_fills_zeroshot_and_leaves_the_tuple_alone(tmp_path, monkeypatch):
    _paths()
    from mmgclip import head
    from mmgclip.experiments.ClassifierExperiment import ClassifierExperiment
    from mmgclip.utils.logger import logger
    plain = _experiment(tmp_path, monkeypatch, []).validate()
    monkeypatch.setattr(head, "_HipAurocBackend", A.TorchAurocBackend)
    lines = []
    monkeypatch.setattr(logger, "info", lambda msg, *a, **k: lines.append(str(msg)))
    exp = _experiment(tmp_path, monkeypatch, ["+experiments/config/zeroshot_auroc=bootstrap", "experiments.config.zeroshot_auroc.n_bootstrap=32"])
    exp.current_epoch = 2
    val = exp.validate()
    assert val == plain
    z = exp.zeroshot
    assert list(z) == ["birads", "malig", "shapes"] and list(z["shapes"]["classes"]) == [0, 1, 2, 3] and list(z["malig"]["classes"]) == [1]
    assert list(z["birads"]["classes"]) == [-1, 0, 1, 2, 3, 4, 5, 6]          # prompt 0 is "unknown" = -1, a negative of every other class
    assert abs(z["malig"]["auc"] - val[1]) <= 1e-12 and abs(z["shapes"]["auc"] - val[2]) <= 1e-12 and abs(z["birads"]["auc"] - val[3]) <= 1e-12
    assert z["malig"]["n_valid"] == 32 and z["malig"]["ci_lower"] <= z["malig"]["ci_upper"]
    new = {k: v for k, v in exp.writer.seen.items() if k.startswith("auc_global/")}
    assert new == {f"auc_global/val/{n}{s}": (z[n][k], 3) for n in z for s, k in (("", "auc"), ("_ci_lower", "ci_lower"), ("_ci_upper", "ci_upper"))}
    assert set(exp.writer.seen) - set(new) == {"loss/val", "auc/val/malig", "auc/val/shapes", "auc/val/birads", "auc/val/average"}
    mine = [l for l in lines if l.startswith("auc_global/val ")]
    assert len(mine) == 1 and "malig" in mine[0] and "shapes" in mine[0] and "birads" in mine[0]
    with pytest.raises(ValueError, match="unknown keys"):
        _experiment(tmp_path, monkeypatch, ["+experiments/config/zeroshot_auroc=bootstrap", "+experiments.config.zeroshot_auroc.replicates=3"])
    assert ClassifierExperiment._auc([0, 1, 1, 0], [0.1, 0.9, 0.2, 0.2]) == 0.875


def test_evaluator_device_route_gives_the_reference_keys_from_the_kernel(monkeypatch):
    """`ci="device"`: the same result keys, the per-prompt auc and the interval from the (emulated) kernel, reproducible from the seed;
    `ci="host"` is the loop it was."""
    _paths()
    from mmgclip import evaluator, head
    monkeypatch.setattr(head, "_HipAurocBackend", A.TorchAurocBackend)
    g = np.random.default_rng(4)
    n = 60
    y = (g.random(n) < 0.4).astype(np.int64)
    sims = g.standard_normal((n, 2)).astype(np.float32)
    sims[:, 1] += y
    ev = evaluator.Evaluator.__new__(evaluator.Evaluator)
    ev.config, ev.device = {"dataset": {"eval": {"bootstrap_ci": {"ci": "device", "seed": 3}}}}, torch.device("cpu")
    ev.prompt_similarities = lambda emb, prompts, use_logits=True: sims
    classes = dict(evaluator.ENUMS["HasMassLabels"])
    names = [{"HasMassLabels": "mass" if v else "nomass"} for v in y]
    import inspect
    sig = inspect.signature(evaluator.Evaluator.zeroshot_label_prompt).parameters
    assert (sig["ci"].default, sig["seed"].default) == ("host", 0) and ev.bootstrap_ci_config() == {"ci": "device", "seed": 3}
    dev = ev.zeroshot_label_prompt(None, names, classes, "HasMassLabels", n_iterations=40, **ev.bootstrap_ci_config())
    assert dev == ev.zeroshot_label_prompt(None, names, classes, "HasMassLabels", n_iterations=40, ci="device", seed=3)
    assert dev != ev.zeroshot_label_prompt(None, names, classes, "HasMassLabels", n_iterations=40, ci="device")          # seed 0
    host = ev.zeroshot_label_prompt(None, names, classes, "HasMassLabels", n_iterations=40, ci="host")
    assert list(dev) == list(host)
    from scipy.special import softmax
    p = softmax(sims, axis=1)
    want = A.reference({"k": (p, y, [0, 1])}, 40, 3)["k"]["classes"]
    prompts = evaluator.label_prompts("HasMassLabels", classes)
    assert [dev[q]["auc"] for q in prompts] == [want[0]["auc"], want[1]["auc"]]
    assert (dev["auc_ci_mean"], dev["auc_ci_lower"], dev["auc_ci_higher"]) == (want[1]["ci_mean"], want[1]["ci_lower"], want[1]["ci_upper"])
    assert all(abs(dev[q]["auc"] - host[q]["auc"]) <= 1e-12 and dev[q]["accuracy"] == host[q]["accuracy"] for q in prompts)
    assert dev["accuracy"] == host["accuracy"] and dev["f1score"] == host["f1score"]
    with pytest.raises(ValueError, match="ci must be"):
        ev.zeroshot_label_prompt(None, names, classes, "HasMassLabels", ci="gpu")


def test_bad_arguments_are_rejected_without_a_gpu():
    """Validation comes before any HIP call: null pointers, sizes, strides, alignment."""
    _paths()
    import ctypes

    from mmgclip import _hip
    lib = _hip.load()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)

    def pairs(sp=p, sn=p, wp=p, ldp=16, wn=p, ldn=16, P=1, Nn=1, B=1, out=p):
        return lib.mmg_auroc_pairs(sp, sn, wp, ldp, wn, ldn, P, Nn, B, out, None)
    for kw, msg in ((dict(sp=None), b"null pointer"), (dict(sn=None), b"null pointer"), (dict(wp=None), b"null pointer"),
                    (dict(wn=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(P=0), b"must be positive"), (dict(Nn=0), b"must be positive"), (dict(B=-1), b"must be positive"),
                    (dict(ldp=8), b"ldw_pos"), (dict(ldp=24), b"ldw_pos"), (dict(P=17), b"ldw_pos"), (dict(ldp=0), b"ldw_pos"),
                    (dict(ldn=20), b"ldw_neg"), (dict(Nn=17), b"ldw_neg"), (dict(Nn=33, ldn=32), b"ldw_neg"),
                    (dict(sn=odd), b"16-byte aligned"), (dict(wn=odd), b"16-byte aligned")):
        assert pairs(**kw) != 0, kw
        assert msg in lib.mmg_last_error(), (kw, lib.mmg_last_error())

    def boot(n=1, b0=0, B=1, w=p, ldw=16):
        return lib.mmg_bootstrap_weights(0, n, b0, B, w, ldw, None)
    for kw, msg in ((dict(w=None), b"null pointer"), (dict(n=0), b"must be positive"), (dict(B=0), b"must be positive"),
                    (dict(b0=-1), b"must be positive"), (dict(b0=2147483647), b"must be positive"), (dict(B=65536), b"65535"),
                    (dict(n=17), b"ldw"), (dict(ldw=8), b"ldw"), (dict(ldw=24, n=20), b"ldw"), (dict(w=odd), b"16-byte aligned")):
        assert boot(**kw) != 0, kw
        assert msg in lib.mmg_last_error(), (kw, lib.mmg_last_error())
