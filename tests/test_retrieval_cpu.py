"""The retrieval metrics, CPU side: `retrieval.RetrievalMetrics` over gloo with world sizes 2 and 4 and UNEVEN shards in all three
`positives` modes (the device arithmetic `head._HipRetrievalBackend` replaced, inside the worker processes only, by the fp32 emulation
of tests/retrieval_ref.py and the clustering by the torch stand-in of tests/test_averaged_fused_cpu.py; Comm and RetrievalMetrics are
the product code), the key construction for `text`, the config surface and its wiring into `ClassifierExperiment.validate()`, and the
library's argument checks.  The inputs are from the exact regime, so every comparison of metrics is `==`."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import retrieval_ref as R
from tests.test_averaged_fused_cpu import THRESHOLD, TorchAveragedBackend, _free_port, _paths, assert_threshold_margin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "mmg-clip_amd", "configs")
N, D, KS = 75, 32, (1, 5, 10)
MODES = ("diagonal", "text", "clusters")


def _shards(world):
    """Uneven on purpose: [39, 36] and [27, 17, 16, 15] of the 75."""
    c = [N // world - r for r in range(world)]
    c[0] += N - sum(c)
    return c


def _want(mode, img, txt, group):
    """The unsharded float64 reference; for `clusters` the labels are the oracle's greedy-threshold clusters in float64."""
    if mode == "diagonal":
        return R.reference_metrics(img, txt, None, KS)
    if mode == "text":
        return R.reference_metrics(img, txt, group, KS)
    from oracle import clip_oracle as O
    assert_threshold_margin(txt)
    e = torch.nn.functional.normalize(txt.double(), dim=1)
    return R.reference_metrics(img, txt, torch.tensor(O.assign_labels(e @ e.t(), THRESHOLD), dtype=torch.int64), KS)


def _install(head):
    head._HipRetrievalBackend = R.TorchRetrievalBackend
    head._HipAveragedBackend = TorchAveragedBackend


def _feed(metrics, img, txt, ids, batch):
    for a in range(0, img.shape[0], batch):
        metrics.update(img[a:a + batch], txt[a:a + batch], ids[a:a + batch])


def _worker(rank, world, port, mode, q):
    _paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from mmgclip import distributed, head, retrieval
    comm = distributed.init_from_env("gloo")
    img, txt, ids, _ = R.exact_pairs(N, D)
    counts = _shards(world)
    sl = slice(sum(counts[:rank]), sum(counts[:rank + 1]))
    _install(head)                                            # this worker process only
    m = retrieval.RetrievalMetrics(ks=KS, positives=mode, similarity_threshold=THRESHOLD, comm=comm)
    # batches of 16 with a ragged last one; the ids arrive 4, 5 or 6 wide depending on the rank (their tail is padding)
    _feed(m, img[sl], txt[sl], ids[sl][:, :4 + rank % 3], 16)
    out = m.compute()
    q.put(dict(rank=rank, metrics=out, calls=comm.report()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_metrics_equal_the_unsharded_reference_gloo(world, mode):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, mode, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    img, txt, _, group = R.exact_pairs(N, D)
    want = _want(mode, img, txt, group)
    assert want["i2t_n_queries"] == N and 0.0 < want["i2t_ties"] and 0.0 < want["i2t_R@1"] < 1.0
    longest = max(_shards(world))
    for r in results:
        assert r["metrics"] == want, (r["rank"], r["metrics"], want)
        c = r["calls"]       # the shard sizes, the two stacks (text: the id width and the ids too); ONE all-reduce of the integers
        assert c["all_gather_calls"] == (5 if mode == "text" else 3) and c["all_reduce_calls"] == 1, c
        assert c["all_reduce_bytes"] == 2 * (N + 3) * 8, c
        width = max(4 + k % 3 for k in range(world))          # the widest ids any rank holds
        ids_bytes = world * (8 + longest * width * 8) if mode == "text" else 0
        assert c["all_gather_bytes"] == world * (8 + 2 * longest * D * 4) + ids_bytes, c


@pytest.mark.parametrize("mode", MODES)
def test_unsharded_metrics_in_batches_equal_the_reference(mode, monkeypatch):
    _paths()
    from mmgclip import head, retrieval
    monkeypatch.setattr(head, "_HipRetrievalBackend", R.TorchRetrievalBackend)
    monkeypatch.setattr(head, "_HipAveragedBackend", TorchAveragedBackend)
    img, txt, ids, group = R.exact_pairs(150, 64)
    m = retrieval.RetrievalMetrics(ks=[10, 1, 5], positives=mode, similarity_threshold=THRESHOLD)
    _feed(m, img, txt, ids, 64)                                # 64 / 64 / 22
    got = m.compute()
    assert got == _want(mode, img, txt, group)
    assert list(got)[:3] == ["i2t_R@1", "i2t_R@5", "i2t_R@10"]
    if mode != "diagonal":                                     # duplicates of the right report stop counting against the model
        assert got["i2t_R@1"] > R.reference_metrics(img, txt, None, KS)["i2t_R@1"]


def test_a_collapsed_model_scores_zero(monkeypatch):
    _paths()
    from mmgclip import head, retrieval
    monkeypatch.setattr(head, "_HipRetrievalBackend", R.TorchRetrievalBackend)
    m = retrieval.RetrievalMetrics()
    m.update(torch.ones(40, 32), torch.ones(40, 32))
    got = m.compute()
    assert got["i2t_R@1"] == got["i2t_R@10"] == got["t2i_R@5"] == 0.0 and got["i2t_ties"] == 1.0 and got["t2i_median_rank"] == 40.0


def test_text_keys_group_identical_token_ids(monkeypatch):
    """Rows of identical token ids share a key, whatever width their batch arrived in; the same keys serve both directions."""
    _paths()
    from mmgclip import head, retrieval
    seen = []

    class Spy:
        @staticmethod
        def rank(x_loc, y_all, row_key, col_label, diag_off):
            seen.append((row_key.clone(), col_label.clone(), diag_off))
            return R.emulate(x_loc, y_all, row_key, col_label, diag_off)
    monkeypatch.setattr(head, "_HipRetrievalBackend", Spy)
    ids_a = torch.tensor([[101, 7, 102, 0], [101, 8, 102, 0], [101, 7, 9, 102]])
    ids_b = torch.tensor([[101, 7, 102], [101, 7, 9], [101, 8, 102]])          # narrower: rows 0 and 2 repeat rows 0 and 1 of ids_a
    g = torch.Generator().manual_seed(0)
    emb = [torch.randint(-2, 3, (3, 32), generator=g).float() for _ in range(4)]
    m = retrieval.RetrievalMetrics(ks=(1,), positives="text")
    m.update(emb[0], emb[1], ids_a)
    m.update(emb[2], emb[3], ids_b)
    out = m.compute()
    assert len(seen) == 2 and all(torch.equal(k, l) and off == 0 for k, l, off in seen) and torch.equal(seen[0][1], seen[1][1])
    lab = seen[0][1].tolist()
    same = [[lab[i] == lab[j] for j in range(6)] for i in range(6)]
    groups = [0, 1, 2, 0, 3, 1]                                  # (101 7 9 | pad) is not (101 7 9 102)
    assert same == [[groups[i] == groups[j] for j in range(6)] for i in range(6)] and seen[0][1].dtype == torch.int64
    assert out["i2t_n_queries"] == 6 and out["i2t_no_positive"] == 0
    with pytest.raises(ValueError, match="token ids"):
        retrieval.RetrievalMetrics(positives="text").update(emb[0], emb[1])


def test_config_fields_are_parsed_and_bad_ones_rejected():
    _paths()
    from mmgclip import retrieval
    from mmgclip.config import compose
    cfg = compose(CFG_DIR, "train_binary_class_clf", [])
    assert "retrieval" not in cfg.experiments.config and retrieval.parse_config(None) is None
    for name in ("train_binary_class_clf", "train_prompt_clf"):           # the shipped example, selected like augment=mammo
        cfg = compose(CFG_DIR, name, ["+experiments/config/retrieval=recall"])
        node = cfg.experiments.config.retrieval
        assert (node.ks, node.positives, node.similarity_threshold) == ([1, 5, 10], "text", 0.65)
        assert cfg.experiments.config.experiment_name and "metrics" in cfg.experiments.config       # the group's own keys are still there
        assert retrieval.parse_config(node) == dict(ks=[1, 5, 10], positives="text", similarity_threshold=0.65)
    cfg = compose(CFG_DIR, "train_binary_class_clf", ["+experiments/config/retrieval=recall", "experiments.config.retrieval.ks=[1,20]",
                                                      "experiments.config.retrieval.positives=clusters",
                                                      "experiments.config.retrieval.similarity_threshold=0.5"])
    m = retrieval.RetrievalMetrics(**retrieval.parse_config(cfg.experiments.config.retrieval))
    assert (m.ks, m.positives, m.similarity_threshold, m.comm) == ((1, 20), "clusters", 0.5, None)
    assert retrieval.parse_config({"positives": "diagonal"}) == {"positives": "diagonal"}
    d = retrieval.RetrievalMetrics()
    assert (d.ks, d.positives, d.similarity_threshold) == ((1, 5, 10), "diagonal", 0.65)
    for bad in ("cluster", "", 3):
        with pytest.raises(ValueError, match="positives"):
            retrieval.parse_config({"positives": bad})
    for bad in ([], [0], [1, -5], [1.5], "10", 10, [1, 1], [True]):
        with pytest.raises(ValueError, match="ks"):
            retrieval.parse_config({"ks": bad})
    with pytest.raises(ValueError, match="unknown keys"):
        retrieval.parse_config({"k": [1]})
    with pytest.raises(ValueError, match="mapping"):
        retrieval.parse_config("text")


class _TinyPairs(torch.nn.Module):
    """A model whose forward hands the batch's embeddings back: validate()'s loop without towers."""

    def __init__(self, config=None):
        super().__init__()
        self.text_encoder = torch.nn.Linear(16, 8, bias=False)
        self.logit_scale = torch.nn.Parameter(torch.tensor(2.0))

    def count_parameters(self, model):
        return 0

    def forward(self, batch, **kw):
        return {"image_embeddings": batch["img"], "text_embeddings": batch["txt"], "logit_scale": self.logit_scale}


class _Scalars:
    def __init__(self):
        self.seen = {}

    def add_scalar(self, name, value, step):
        self.seen[name] = (value, step)


def _experiment(tmp_path, monkeypatch, extra):
    from mmgclip.config import compose
    from mmgclip.experiments import ClassifierExperiment as CE
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(CE, "model", _TinyPairs)
    over = [f"checkpoints.checkpoints_export_dir={tmp_path}", f"base.tensorboard_export_dir={tmp_path}", "experiments.config.metrics=[]"]
    img, txt, ids, group = R.exact_pairs(150, 64)
    loader = [dict(img=img[a:a + 64], txt=txt[a:a + 64], text_tokens={"input_ids": ids[a:a + 64]}, prompt_labels=[])
              for a in range(0, 150, 64)]
    exp = CE.ClassifierExperiment(config=compose(CFG_DIR, "train_binary_class_clf", over + list(extra)), train_dataloader=[],
                                  valid_dataloader=loader)
    exp.criterion = lambda **out: (out["image_embeddings"].sum() * 0 + 1.5, None)
    exp.writer = _Scalars()
    return exp, (img, txt, group)


def test_validate_without_the_key_makes_no_retrieval_metrics(tmp_path, monkeypatch):
    _paths()
    from mmgclip import retrieval

    class Forbidden:
        def __init__(self, *a, **k):
            raise AssertionError("validate() built a RetrievalMetrics although experiments.config.retrieval is absent")
    monkeypatch.setattr(retrieval, "RetrievalMetrics", Forbidden)
    for extra in ([], ["+experiments.config.retrieval=null"]):
        exp, _ = _experiment(tmp_path, monkeypatch, extra)
        assert exp.validate() == (1.5, -1, -1, -1, -1) and exp.retrieval is None
        assert set(exp.writer.seen) == {"loss/val"}


def test_validate_with_the_key_fills_retrieval_and_leaves_the_tuple_alone(tmp_path, monkeypatch):
    _paths()
    from mmgclip import head
    from mmgclip.utils.logger import logger
    monkeypatch.setattr(head, "_HipRetrievalBackend", R.TorchRetrievalBackend)
    lines = []
    monkeypatch.setattr(logger, "info", lambda msg, *a, **k: lines.append(str(msg)))
    exp, (img, txt, group) = _experiment(tmp_path, monkeypatch, ["+experiments/config/retrieval=recall", "experiments.config.retrieval.ks=[1,5]"])
    exp.current_epoch = 2
    assert exp.validate() == (1.5, -1, -1, -1, -1)
    want = R.reference_metrics(img, txt, group, (1, 5))
    assert exp.retrieval == want
    assert {k: v for k, v in exp.writer.seen.items() if k != "loss/val"} == {f"retrieval/val/{k}": (v, 3) for k, v in want.items()}
    mine = [l for l in lines if l.startswith("retrieval/val ")]
    assert len(mine) == 1 and "i2t_R@1" in mine[0] and "t2i_mrr" in mine[0]
    with pytest.raises(ValueError, match="positives"):
        _experiment(tmp_path, monkeypatch, ["+experiments/config/retrieval=recall", "experiments.config.retrieval.positives=nearest"])


def test_bad_arguments_are_rejected_without_a_gpu():
    """Validation comes before any HIP call: D, sizes, null pointers, a key without its labels (and the reverse), a diagonal that
    leaves the gallery."""
    _paths()
    import ctypes

    from mmgclip import _hip
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def rank(X=p, Y=p, key=None, lab=None, n=1, N=1, D=32, off=0, best=p, n_pos=p, n_gt=p, n_eq=p):
        return lib.mmg_retrieval_rows_rank(X, Y, key, lab, n, N, D, off, best, n_pos, n_gt, n_eq, None)
    for kw, msg in ((dict(D=100), b"multiple of 32"), (dict(D=2048), b"multiple of 32"), (dict(D=0), b"multiple of 32"),
                    (dict(n=0), b"must be positive"), (dict(N=-3), b"must be positive"),
                    (dict(X=None), b"null pointer"), (dict(Y=None), b"null pointer"), (dict(best=None), b"null pointer"),
                    (dict(n_pos=None), b"null pointer"), (dict(n_gt=None), b"null pointer"), (dict(n_eq=None), b"null pointer"),
                    (dict(key=p), b"come together"), (dict(lab=p), b"come together"),
                    (dict(off=-1), b"diag_off + n_loc <= N"), (dict(off=1), b"diag_off + n_loc <= N"),
                    (dict(n=4, N=3), b"diag_off + n_loc <= N"), (dict(n=2, N=8, off=7), b"diag_off + n_loc <= N"),
                    (dict(n=1, N=8, off=2147483647), b"diag_off + n_loc <= N")):
        assert rank(**kw) != 0, kw
        assert msg in lib.mmg_last_error(), (kw, lib.mmg_last_error())
