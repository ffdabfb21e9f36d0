"""The nearest-neighbour search, CPU side: `search.EmbeddingIndex` over gloo with world sizes 2 and 4 and UNEVEN gallery and query
shards in all three exclusion modes (the device arithmetic `head._HipTopKBackend` replaced, inside the worker processes only, by the
fp32 emulation of tests/topk_ref.py; Comm, EmbeddingIndex and merge_topk are the product code), `chunk_rows`, `ReportRetriever` on a
tiny stand-in model, the index's argument checks, and the library's argument checks and support table.  The inputs are from the exact
regime, so every comparison is torch.equal."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import topk_ref as T
from tests.test_averaged_fused_cpu import _free_port, _paths

NQ, N, D, K, OFF = 53, 75, 32, 10, 4


def _shards(total, world):
    """Uneven on purpose: [39, 36] and [27, 17, 16, 15] of 75."""
    c = [total // world - r for r in range(world)]
    c[0] += total - sum(c)
    return c


def _problem(mode):
    """Queries, gallery, (row_key, col_label), the excluded mask of the UNSHARDED search and the `exclude` argument builder."""
    X, Y = T.exact_case(NQ, N, D, OFF)
    if mode == "none":
        return X, Y, None, None, torch.zeros(NQ, N, dtype=torch.bool)
    if mode == "diagonal":
        return X, Y, None, None, T.positive_mask(NQ, N, OFF)
    lab = T.hand_labels(N)
    key = lab[OFF + torch.arange(NQ)].clone()
    key[5] = T.ABSENT_KEY
    return X, Y, key, lab, T.positive_mask(NQ, N, 0, key, lab)


def _exclude(mode, key, lab):
    return None if mode == "none" else ("diagonal", OFF) if mode == "diagonal" else ("labels", key, lab)


def _want(mode):
    X, Y, _, _, excluded = _problem(mode)
    r = T.reference(X, Y, K, excluded)
    return r.scores.float(), r.indices


def _worker(rank, world, port, mode, q):
    _paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from mmgclip import distributed, head, search
    comm = distributed.init_from_env("gloo")
    X, Y, key, lab, _ = _problem(mode)
    gc, qc = _shards(N, world), _shards(NQ, world)[::-1]            # the gallery's and the queries' shards differ
    gs = slice(sum(gc[:rank]), sum(gc[:rank + 1]))
    qs = slice(sum(qc[:rank]), sum(qc[:rank + 1]))
    head._HipTopKBackend = T.TorchTopKBackend                      # this worker process only
    index = search.EmbeddingIndex(Y[gs].contiguous(), comm=comm, chunk_rows=7 if rank % 2 else None)
    built = comm.report()
    scores, indices = index.search(X[qs].contiguous(), K, _exclude(mode, None if key is None else key[qs], None if lab is None else lab[gs]))
    q.put(dict(rank=rank, rows=(qs.start, qs.stop), scores=scores, indices=indices, built=built, calls=comm.report(), total=len(index)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_search_equals_the_unsharded_reference_gloo(world, mode):
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
    want_s, want_j = _want(mode)
    assert bool((want_s[:, :-1] == want_s[:, 1:]).any())             # ties that only the index decides, across shards too
    longest = max(_shards(NQ, world))
    for r in results:
        a, b = r["rows"]
        assert r["scores"].dtype == torch.float32 and r["indices"].dtype == torch.int64 and r["total"] == N
        assert torch.equal(r["scores"], want_s[a:b]) and torch.equal(r["indices"], want_j[a:b]), (r["rank"], mode)
        # the row counts once at construction; per search the query counts, the queries (labels: and their keys), the two lists
        assert r["built"]["all_gather_calls"] == 1 and r["built"]["all_reduce_calls"] == 0, r["built"]
        c = r["calls"]
        assert c["all_gather_calls"] == (5 if mode == "labels" else 4) and c["all_reduce_calls"] == 0, c
        keys = world * longest * 8 if mode == "labels" else 0
        assert c["all_gather_bytes"] == world * (8 + longest * D * 4 + 2 * NQ * K * 4) + keys, c


@pytest.mark.parametrize("mode", T.MODES)
def test_unsharded_search_and_chunk_rows_equal_the_reference(mode, monkeypatch):
    _paths()
    from mmgclip import head, search
    monkeypatch.setattr(head, "_HipTopKBackend", T.TorchTopKBackend)
    X, Y, key, lab, _ = _problem(mode)
    want = _want(mode)
    for chunk in (None, 1, 7, 32, N, 1000):
        got = search.EmbeddingIndex(Y, chunk_rows=chunk).search(X, K, _exclude(mode, key, lab))
        assert got[1].dtype == torch.int64 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), chunk
    wide = search.EmbeddingIndex(Y[:6].contiguous(), chunk_rows=4).search(X, 8)            # k > N: padded
    assert bool((wide[1][:, 6:] == -1).all()) and bool((wide[0][:, 6:] == T.NINF).all()) and bool((wide[1][:, :6] >= 0).all())


def test_the_index_rejects_what_it_cannot_search(monkeypatch):
    _paths()
    from mmgclip import head, search
    monkeypatch.setattr(head, "_HipTopKBackend", T.TorchTopKBackend)
    X, Y = T.exact_case(8, 40, 64, 0)
    index = search.EmbeddingIndex(Y)
    for k in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="positive integer"):
            index.search(X, k)
    with pytest.raises(ValueError, match="limit of 32"):
        index.search(X, 33)
    big = search.EmbeddingIndex(torch.zeros(4, 1024))
    with pytest.raises(ValueError, match="D=1024 with k=32"):
        big.search(torch.zeros(2, 1024), 32)
    assert big.search(torch.zeros(2, 1024), 16)[1].tolist() == [[0, 1, 2, 3] + [-1] * 12] * 2      # equal scores: the index decides
    with pytest.raises(ValueError, match="D=48 with k=4"):
        search.EmbeddingIndex(torch.zeros(4, 48)).search(torch.zeros(2, 48), 4)
    with pytest.raises(ValueError, match="contiguous"):
        index.search(X.t().contiguous().t(), 3)
    with pytest.raises(ValueError, match="contiguous"):
        search.EmbeddingIndex(Y[:, ::2])
    with pytest.raises(ValueError, match="fp32"):
        index.search(X.bfloat16(), 3)
    with pytest.raises(ValueError, match="fp32"):
        search.EmbeddingIndex(Y.bfloat16())
    with pytest.raises(ValueError, match=r"\[rows,D\]"):
        search.EmbeddingIndex(Y[0])
    with pytest.raises(ValueError, match="D=32"):
        index.search(torch.zeros(2, 32), 3)
    with pytest.raises(ValueError, match="chunk_rows"):
        search.EmbeddingIndex(Y, chunk_rows=0)
    for bad in ("diagonal", ("diagonal",), ("diagonal", -1), ("nearest", 0), ("labels", torch.zeros(8, dtype=torch.int64)),
                ("labels", torch.zeros(8, dtype=torch.int32), torch.zeros(40, dtype=torch.int64)),
                ("labels", torch.zeros(8, dtype=torch.int64), torch.zeros(39, dtype=torch.int64))):
        with pytest.raises(ValueError, match="exclude|row_key|col_label"):
            index.search(X, 3, bad)


class _TinyModel(torch.nn.Module):
    """A model whose towers are look-ups: report j's text features are row j of an integer table (its one token id is j), image
    features pass through."""

    class _Cfg:
        pass

    def __init__(self, table, project):
        super().__init__()
        self.device = torch.device("cpu")
        self.table = table
        cfg = self._Cfg()
        cfg.tokenizer = self._Cfg()
        cfg.tokenizer.config = self._Cfg()
        cfg.tokenizer.config.tokenizer_name, cfg.tokenizer.config.sequence_length = "none", 4
        self.config = cfg
        self.text_projection_layer = self.image_projection_layer = None
        if project:                                                # an integer "projection": exactness survives it
            self.text_projection_layer = lambda f: 2.0 * f
            self.image_projection_layer = lambda f: f.flip(1)
        self.batches = []

    def encode_text(self, batch, text_pooling="eos"):
        assert text_pooling == "eos" and not self.training and not torch.is_grad_enabled()
        ids = batch["text_tokens"]["input_ids"]
        self.batches.append(ids.shape[0])
        return self.table[ids[:, 0]]

    def encode_images(self, batch):
        assert not self.training and not torch.is_grad_enabled()
        return batch["image_features"]


class _Identity:
    apply = staticmethod(lambda x: x)


@pytest.mark.parametrize("project", [False, True])
def test_report_retriever_returns_the_strings_of_the_reference(project, monkeypatch):
    _paths()
    from mmgclip import head
    from mmgclip.networks.mmgclip_model import PromptClassifier, ReportRetriever
    monkeypatch.setattr(head, "_HipTopKBackend", T.TorchTopKBackend)
    monkeypatch.setattr(head, "L2Normalize", _Identity)           # the table's rows stand for normalised embeddings
    X, Y = T.exact_case(9, 70, 64, 0)
    texts = [f"report {j}" for j in range(70)]
    seen = []

    def tokenizer(strings, padding, truncation, return_tensors, max_length):
        seen.append((len(strings), padding, truncation, return_tensors, max_length))
        return {"input_ids": torch.tensor([[int(s.split()[1]), 0, 0, 0] for s in strings])}
    model = _TinyModel(Y, project).train()
    rr = ReportRetriever(model, tokenizer=tokenizer)
    assert isinstance(rr, PromptClassifier) and ReportRetriever._tokens is PromptClassifier._tokens
    with pytest.raises(RuntimeError, match="build"):
        rr(X)
    assert rr.build(texts, batch_size=32) is rr
    assert model.batches == [32, 32, 6] and seen == [(b, "max_length", True, "pt", 4) for b in (32, 32, 6)]
    gallery = 2.0 * Y if project else Y
    assert torch.equal(rr.index.embeddings, gallery) and len(rr.index) == 70
    queries = X.flip(1) if project else X
    for k in (5, 1):
        out = rr(X, k=k) if k != 5 else rr(X)
        r = T.reference(queries, gallery, k, torch.zeros(9, 70, dtype=torch.bool))
        assert set(out) == {"indices", "scores", "texts"}
        assert out["indices"].dtype == torch.int64 and torch.equal(out["indices"], r.indices) and torch.equal(out["scores"], r.scores.float())
        assert out["texts"] == [[texts[j] for j in row] for row in r.indices.tolist()]
    few = ReportRetriever(model, tokenizer=tokenizer).build(texts[:3])(X, k=4)
    assert all(row[3] is None and row[:3] == [texts[j] for j in idx[:3]] for row, idx in zip(few["texts"], few["indices"].tolist()))
    with pytest.raises(ValueError, match="strings"):
        rr.build([])


def test_bad_arguments_are_rejected_without_a_gpu():
    """Validation comes before any HIP call: the dims, k, the support table, the exclusion mode and its pointer rules, j_base, null
    pointers - each with its message."""
    _paths()
    import ctypes

    from mmgclip import _hip
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def topk(X=p, Y=p, n=1, N=1, D=32, k=1, ex=0, key=None, lab=None, off=0, jb=0, acc=0, scores=p, indices=p):
        return lib.mmg_topk_rows(X, Y, n, N, D, k, ex, key, lab, off, jb, acc, scores, indices, None)
    for kw, msg in ((dict(D=100), b"multiple of 32"), (dict(D=2048), b"multiple of 32"), (dict(D=0), b"multiple of 32"),
                    (dict(n=0), b"must be positive"), (dict(N=-3), b"must be positive"),
                    (dict(k=0), b"must be in [1,32]"), (dict(k=33), b"must be in [1,32]"), (dict(k=-1), b"must be in [1,32]"),
                    (dict(D=1024, k=32), b"D=1024 with k=32 is unsupported"),
                    (dict(ex=3), b"exclude=3 must be"), (dict(ex=-1), b"exclude=-1 must be"),
                    (dict(ex=0, key=p), b"must be NULL"), (dict(ex=0, lab=p), b"must be NULL"), (dict(ex=0, key=p, lab=p), b"must be NULL"),
                    (dict(ex=1, key=p), b"must be NULL"), (dict(ex=1, lab=p), b"must be NULL"),
                    (dict(ex=2), b"needs row_key and col_label"), (dict(ex=2, key=p), b"needs row_key and col_label"),
                    (dict(ex=2, lab=p), b"needs row_key and col_label"),
                    (dict(ex=1, off=-1), b"diag_off >= 0"),
                    (dict(jb=-1), b"j_base"), (dict(jb=2147483647), b"j_base"), (dict(jb=2147483000, N=648), b"j_base"),
                    (dict(X=None), b"null pointer"), (dict(Y=None), b"null pointer"), (dict(scores=None), b"null pointer"),
                    (dict(indices=None), b"null pointer"), (dict(acc=1, scores=None), b"null pointer")):
        assert topk(**kw) != 0, kw
        assert msg in lib.mmg_last_error(), (kw, lib.mmg_last_error())


def test_support_table_of_the_library():
    """1 on the guaranteed domain (every D % 32 == 0 up to 768 with k <= 32; up to 1024 with k <= 16); the LDS of a supported plan is
    what the reference derives and never above 160 KB; 0 bytes where unsupported."""
    _paths()
    from mmgclip import _hip, head
    lib = _hip.load()
    for D in list(range(32, 1025, 32)) + [0, 16, 48, 1000, 1056, -32]:
        for k in range(-1, 35):
            ok = lib.mmg_topk_rows_supported(D, k)
            assert ok == int(T.supported(D, k)) and head._HipTopKBackend.supported(D, k) == bool(ok), (D, k)
            nbytes = lib.mmg_topk_rows_lds_bytes(D, k)
            assert nbytes == (T.lds_bytes(D, k) if ok else 0) and nbytes <= 163840, (D, k, nbytes)
            if D > 0 and D % 32 == 0 and 1 <= k and ((D <= 768 and k <= 32) or (D <= 1024 and k <= 16)):
                assert ok == 1, (D, k)
    assert lib.mmg_topk_rows_lds_bytes(768, 32) == 131584 and lib.mmg_topk_rows_supported(1024, 32) == 0
