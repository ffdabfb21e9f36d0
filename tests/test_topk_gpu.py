"""The nearest-neighbour search on the MI355X: the kernel of csrc/topk_head.hip through `_hip.call` on the test's own buffers, then
`EmbeddingIndex` and `ReportRetriever`, against the float64 reference of tests/topk_ref.py.

Every kernel call without `accumulate` writes into buffers pre-filled with NaN bits (scores) or a poison integer (indices) and followed
by 32 sentinel entries; no output may keep its fill and no sentinel may change - a padded row that is written shows there.

Exact regime (torch.equal on scores and indices): integer rows in {-2..2}, topk_ref.EXACT_SHAPES, without exclusion, on the diagonal and
with sigmoid_ref.hand_labels; one labelled case carries a query whose key matches nothing.  The preconditions are asserted on the
inputs alone (topk_ref.exactness_violations; also tests/test_topk_ref_cpu.py).
Gaussian regime: random unit rows, topk_ref.GAUSS_SHAPES; every row passes the checks derived from E_dot = Kd(D) u sum|x||y|, at most
1/8 of a case's rows open."""
import os

import pytest
import torch

from tests import topk_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "mmg-clip_amd", "configs")
TAIL = 32
SENTINEL = 12345
NAN_BITS = 0x7FC00ABC
POISON = -77777


def _launch(dev, X, Y, k, exclude, key, lab, off, j_base=0, prev=None):
    """One launch -> scores fp32 [n,k], indices int32 [n,k] (CPU).  Fresh, poisoned buffers; with `prev` (the CPU lists of earlier
    launches) the buffers hold those and the launch accumulates."""
    from mmgclip._hip import call, ptr, stream
    n, D = X.shape
    Xd, Yd = X.to(dev).contiguous(), Y.to(dev).contiguous()
    kd = None if key is None else key.to(dev).contiguous()
    ld = None if lab is None else lab.to(dev).contiguous()
    scores = torch.full(((n + TAIL) * k,), float(SENTINEL), device=dev, dtype=torch.float32)
    indices = torch.full(((n + TAIL) * k,), SENTINEL, device=dev, dtype=torch.int32)
    if prev is None:
        scores[:n * k].view(torch.int32).fill_(NAN_BITS)
        indices[:n * k] = POISON
    else:
        scores[:n * k] = prev[0].to(dev).reshape(-1)
        indices[:n * k] = prev[1].to(dev).reshape(-1)
    call("mmg_topk_rows", ptr(Xd), ptr(Yd), n, Y.shape[0], D, k, exclude, ptr(kd), ptr(ld), off, j_base, 0 if prev is None else 1,
         ptr(scores), ptr(indices), stream())
    torch.cuda.synchronize()
    assert bool((scores[n * k:] == SENTINEL).all()) and bool((indices[n * k:] == SENTINEL).all()), \
        "a sentinel after the output changed (a padded row was written)"
    s, j = scores[:n * k].reshape(n, k).cpu(), indices[:n * k].reshape(n, k).cpu()
    assert not bool(torch.isnan(s).any()), "an owned score kept its NaN fill (or the kernel produced one)"
    assert not bool((j == POISON).any()), "an owned index kept its fill"
    return s, j


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("shape", T.EXACT_SHAPES)
def test_exact_regime_is_bit_exact(dev, shape, mode):
    X, Y, key, lab, excluded = T.case(shape, mode, "exact")
    assert T.exactness_violations(X, Y) == []
    n, N, D, off, k = shape
    ref = T.reference(X, Y, k, excluded)
    scores, indices = _launch(dev, X, Y, k, T.EXCLUDE[mode], key, lab, off)
    assert torch.equal(indices, ref.indices.int()), torch.nonzero((indices != ref.indices.int()).any(1)).flatten().tolist()
    assert torch.equal(scores, ref.scores.float())
    if mode == "labels" and shape == T.ABSENT_CASE[0]:
        row = T.ABSENT_CASE[1]
        assert torch.equal(indices[row], T.reference(X, Y, k, torch.zeros_like(excluded)).indices.int()[row])


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("shape", T.GAUSS_SHAPES)
def test_gaussian_regime_inside_the_intervals(dev, shape, mode):
    X, Y, key, lab, excluded = T.case(shape, mode, "gauss")
    n, N, D, off, k = shape
    ref = T.intervals(X, Y, k, excluded)
    assert ref.open_share <= T.OPEN_CAP, ref.open_share
    scores, indices = _launch(dev, X, Y, k, T.EXCLUDE[mode], key, lab, off)
    print(shape, mode, "open share", ref.open_share, "decided rows", int(ref.decided.sum()),
          "rows equal to the reference", int((indices == ref.indices.int()).all(1).sum()), "of", n)
    assert T.interval_violations(ref, scores, indices) == []


@pytest.mark.parametrize("mode", T.MODES)
def test_split_launches_chunks_and_repeats_are_bit_identical(dev, mode):
    """(96, 300, 64), k = 32: one launch; three launches over the row blocks 32 / 40 / 24 at their offsets; three gallery chunks of
    128 / 100 / 72 columns through j_base and accumulate; and once more.  All by torch.equal, scores and indices."""
    shape = (96, 300, 64, 0, 32)
    X, Y, key, lab, _ = T.case(shape, mode, "gauss")
    k, ex = shape[4], T.EXCLUDE[mode]
    one = _launch(dev, X, Y, k, ex, key, lab, 0)
    again = _launch(dev, X, Y, k, ex, key, lab, 0)
    rows = [_launch(dev, X[a:b], Y, k, ex, None if key is None else key[a:b], lab, a) for a, b in ((0, 32), (32, 72), (72, 96))]
    chunked = None
    for a, b in ((0, 128), (128, 228), (228, 300)):
        chunked = _launch(dev, X, Y[a:b], k, ex, key, None if lab is None else lab[a:b], 0, j_base=a, prev=chunked)
    for t in range(2):
        assert torch.equal(one[t], again[t])
        assert torch.equal(one[t], torch.cat([p[t] for p in rows]))
        assert torch.equal(one[t], chunked[t])


@pytest.mark.parametrize("mode", T.MODES)
def test_the_index_on_the_device_equals_the_reference(dev, mode):
    """`EmbeddingIndex.search` on exact-regime data, in one launch and streamed with chunk_rows: scores and int64 indices of the
    float64 reference."""
    from mmgclip import search
    n, N, D, off, k = 40, 300, 64, 0, 32
    X, Y, key, lab, excluded = T.case((n, N, D, off, k), mode, "exact")
    ref = T.reference(X, Y, k, excluded)
    exclude = None if mode == "none" else ("diagonal", off) if mode == "diagonal" else ("labels", key.to(dev), lab.to(dev))
    for chunk in (None, 77):
        scores, indices = search.EmbeddingIndex(Y.to(dev), chunk_rows=chunk).search(X.to(dev), k, exclude)
        assert scores.is_cuda and indices.dtype == torch.int64 and scores.dtype == torch.float32
        assert torch.equal(indices.cpu(), ref.indices) and torch.equal(scores.cpu(), ref.scores.float()), chunk


def test_no_dense_matrix_is_allocated(dev):
    """n = 256 queries against N = 4096 rows at D = 64, k = 10: the peak of the allocator above the inputs and the outputs stays
    below 1 MiB; the dense scores alone would be 4 MiB."""
    from mmgclip import head
    n, N, D, k = 256, 4096, 64, 10
    X, Y = T.gaussian_case(n, N, D, 0)
    Xd, Yd = X.to(dev), Y.to(dev)
    head._HipTopKBackend.topk(Xd[:32], Yd[:64], k)                 # the library and the allocator are warm
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    scores, indices = head._HipTopKBackend.topk(Xd, Yd, k)
    torch.cuda.synchronize()
    outputs = scores.numel() * 4 + indices.numel() * 4
    rise = torch.cuda.max_memory_allocated() - base - outputs
    print("rise above inputs and outputs", rise, "bytes; outputs", outputs, "; dense", n * N * 4)
    assert n * N * 4 == 4 * 2 ** 20 and rise < 2 ** 20
    assert bool((indices >= 0).all()) and bool((indices < N).all()) and bool((scores[:, :-1] >= scores[:, 1:]).all())


def _model(monkeypatch):
    """The small 2-layer BERT of the retrieval test's experiment, as a bare MMGCLIP in the `train_prompt_clf` layout (pre-extracted
    image features, 1xLinear512 projections)."""
    from mmgclip.config import compose
    from mmgclip.networks import bert
    from mmgclip.networks.mmgclip_model import MMGCLIP
    orig = bert.BertConfigLite.__init__

    def small(self, **kw):
        kw.setdefault("num_hidden_layers", 2)
        kw.setdefault("vocab_size", 3000)
        orig(self, **kw)
    monkeypatch.setattr(bert.BertConfigLite, "__init__", small)
    cfg = compose(CFG_DIR, "train_binary_class_clf", ["networks.text_encoder.random_init=true", "tokenizer=bert_clinical_seqlen=77"])
    torch.manual_seed(0)
    return MMGCLIP(cfg)


def test_report_retriever_on_the_device(dev, monkeypatch):
    """build() keeps exactly the text embeddings the model's forward returns for the same strings; forward() returns the reference's
    neighbours of the model's image embeddings, and their strings."""
    from mmgclip.dataset.synthetic import synthetic_batch, synthetic_prompt_tokens
    from mmgclip.networks.mmgclip_model import ReportRetriever
    model = _model(monkeypatch)
    texts = [f"finding {j}: " + " ".join(f"w{(7 * j + t) % 41}" for t in range(3 + j % 5)) for j in range(45)]
    rr = ReportRetriever(model, tokenizer=lambda strings, **kw: synthetic_prompt_tokens(strings, kw["max_length"], vocab_size=3000))
    rr.build(texts, batch_size=16)
    feats = synthetic_batch(16, S=77, vocab_size=3000, seed=5)["image_features"]
    model.eval()
    with torch.no_grad():
        out = model({"image_features": feats, "text_tokens": rr._tokens(texts[:16])}, materialize_logits=False)
    assert torch.equal(rr.index.embeddings[:16], out["text_embeddings"].float())        # the first batch of build(): the same launch shapes
    got = rr(feats, k=5)
    E = rr.index.embeddings.cpu()
    Q = out["image_embeddings"].float().cpu()
    ref = T.intervals(Q, E, 5, torch.zeros(16, 45, dtype=torch.bool))
    assert got["indices"].dtype == torch.int64 and got["scores"].dtype == torch.float32
    assert T.interval_violations(ref, got["scores"].cpu(), got["indices"].cpu()) == []
    assert got["texts"] == [[texts[j] for j in row] for row in got["indices"].tolist()]
    assert len(got["texts"]) == 16 and all(len(row) == 5 for row in got["texts"])
