"""The retrieval ranks on the MI355X: the kernel of csrc/retrieval_head.hip through `_hip.call` on the test's own buffers, then
`RetrievalMetrics` and `ClassifierExperiment.validate()`, against the float64 / int64 reference of tests/retrieval_ref.py.

Every kernel call writes into buffers pre-filled with NaN bits (best) or a poison integer (the counts) and followed by 32 sentinel
entries; no output may keep its fill and no sentinel may change - a padded row that is written shows there.

Exact regime (torch.equal on all four outputs, best as fp32): integer rows in {-2..2}, retrieval_ref.EXACT_SHAPES, on the diagonal and
with sigmoid_ref.hand_labels; one labelled case carries a query whose key no gallery row has.  The preconditions are asserted on the
inputs alone (retrieval_ref.exactness_violations; also tests/test_retrieval_ref_cpu.py).
Gaussian regime: random unit rows, retrieval_ref.GAUSS_SHAPES; every row's counts inside the interval derived from
E_dot = Kd(D) u sum|x||y|, equal to the reference where the interval is a point, at most 1/8 of a case's intervals open."""
import os

import numpy as np
import pytest
import torch

from tests import retrieval_ref as R
from tests.test_retrieval_ref_cpu import ABSENT_CASE, _case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "mmg-clip_amd", "configs")
TAIL = 32
SENTINEL = 12345
NAN_BITS = 0x7FC00ABC
POISON = -77777


def _launch(dev, X, Y, key, lab, off):
    """One launch on fresh, poisoned buffers -> best fp32, n_pos, n_gt, n_eq int32 (CPU)."""
    from mmgclip._hip import call, ptr, stream
    n, D = X.shape
    Xd, Yd = X.to(dev).contiguous(), Y.to(dev).contiguous()
    kd = None if key is None else key.to(dev).contiguous()
    ld = None if lab is None else lab.to(dev).contiguous()
    best = torch.full((n + TAIL,), float(SENTINEL), device=dev, dtype=torch.float32)
    best[:n].view(torch.int32).fill_(NAN_BITS)
    counts = [torch.full((n + TAIL,), SENTINEL, device=dev, dtype=torch.int32) for _ in range(3)]
    for c in counts:
        c[:n] = POISON
    call("mmg_retrieval_rows_rank", ptr(Xd), ptr(Yd), ptr(kd), ptr(ld), n, Y.shape[0], D, off, ptr(best), *(ptr(c) for c in counts), stream())
    torch.cuda.synchronize()
    out = []
    for t in [best] + counts:
        assert bool((t[n:] == SENTINEL).all()), "a sentinel after the output changed (a padded row was written)"
        out.append(t[:n].cpu())
    assert not bool(torch.isnan(out[0]).any()), "an owned element of best kept its NaN fill (or the kernel produced one)"
    assert all(not bool((c == POISON).any()) for c in out[1:]), "an owned count kept its fill"
    return tuple(out)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.EXACT_SHAPES)
def test_exact_regime_is_bit_exact(dev, shape, mode):
    X, Y, key, lab, pos = _case(shape, mode, "exact")
    assert R.exactness_violations(X, Y) == []
    ref = R.reference(X, Y, pos)
    best, n_pos, n_gt, n_eq = _launch(dev, X, Y, key, lab, shape[3])
    assert torch.equal(n_pos, ref.n_pos.int())
    assert torch.equal(best, ref.best.float())
    assert torch.equal(n_gt, ref.n_gt.int()), torch.nonzero(n_gt != ref.n_gt.int()).flatten().tolist()
    assert torch.equal(n_eq, ref.n_eq.int()), torch.nonzero(n_eq != ref.n_eq.int()).flatten().tolist()
    if mode == "labels" and shape == ABSENT_CASE[0]:
        row = ABSENT_CASE[1]
        assert int(n_pos[row]) == 0 and float(best[row]) == float("-inf") and int(n_gt[row]) == shape[1] and int(n_eq[row]) == 0


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.GAUSS_SHAPES)
def test_gaussian_regime_inside_the_intervals(dev, shape, mode):
    X, Y, key, lab, pos = _case(shape, mode, "gauss")
    ref = R.intervals(X, Y, pos)
    assert ref.open_share <= R.OPEN_CAP, ref.open_share
    got = _launch(dev, X, Y, key, lab, shape[3])
    print(shape, mode, "open share", ref.open_share, "ties", int((got[3] > 0).sum()))
    assert R.interval_violations(ref, *got) == []


@pytest.mark.parametrize("mode", R.MODES)
def test_split_launches_equal_one_launch_and_runs_repeat(dev, mode):
    """(96, 300, 64): the rows as one launch, as three launches of 32 / 40 / 24 rows at their offsets, and once more: a query's
    results do not depend on the rows that share its launch, and nothing varies from run to run."""
    shape = (96, 300, 64, 0)
    X, Y, key, lab, _ = _case(shape, mode, "gauss")
    one = _launch(dev, X, Y, key, lab, 0)
    again = _launch(dev, X, Y, key, lab, 0)
    parts = [_launch(dev, X[a:b], Y, None if key is None else key[a:b], lab, a) for a, b in ((0, 32), (32, 72), (72, 96))]
    for k in range(4):
        assert torch.equal(one[k], again[k]) and torch.equal(one[k], torch.cat([p[k] for p in parts]))


@pytest.mark.parametrize("mode", ("diagonal", "text", "clusters"))
def test_metrics_on_the_device_equal_the_reference(dev, mode):
    """150 exact-regime pairs with planted duplicate texts, fed as 64 / 64 / 22: the metric dict equals the float64 reference's
    (for `clusters`: on the oracle's greedy-threshold clusters of the same text, which sit far from the threshold)."""
    from mmgclip import retrieval
    from oracle import clip_oracle as O
    from tests.test_averaged_fused_cpu import THRESHOLD, assert_threshold_margin
    img, txt, ids, group = R.exact_pairs(150, 64)
    labels = None
    if mode == "text":
        labels = group
    elif mode == "clusters":
        assert_threshold_margin(txt)
        e = torch.nn.functional.normalize(txt.double(), dim=1)
        labels = torch.tensor(O.assign_labels(e @ e.t(), THRESHOLD), dtype=torch.int64)
    want = R.reference_metrics(img, txt, labels, (1, 5, 10))
    m = retrieval.RetrievalMetrics(ks=(1, 5, 10), positives=mode, similarity_threshold=THRESHOLD)
    for a in range(0, 150, 64):
        m.update(img[a:a + 64].to(dev), txt[a:a + 64].to(dev), ids[a:a + 64].to(dev))
    got = m.compute()
    print(mode, got)
    assert got == want
    assert 0.0 < got["i2t_ties"] and 0.0 < got["i2t_R@1"] < 1.0 and got["i2t_n_queries"] == 150 and got["i2t_no_positive"] == 0


def _experiment(monkeypatch, tmp_path, extra):
    from mmgclip.config import compose
    from mmgclip.dataset.synthetic import SyntheticLoader
    from mmgclip.experiments.experiments_controller import create_experiment
    from mmgclip.networks import bert
    orig = bert.BertConfigLite.__init__

    def small(self, **kw):
        kw.setdefault("num_hidden_layers", 2)
        kw.setdefault("vocab_size", 3000)
        orig(self, **kw)
    monkeypatch.setattr(bert.BertConfigLite, "__init__", small)
    # loss=sigmoid: its validation loss has one owner per row and a fixed tree, so two runs can be compared with `==`; the dense
    # CLIPLoss validate() uses adds its rows with float atomics (mmg_ce_rows_fwd) and its last bit varies from run to run
    cfg = compose(CFG_DIR, "train_binary_class_clf", ["networks.text_encoder.random_init=true", "tokenizer=bert_clinical_seqlen=77",
                                                      "loss=sigmoid"] + list(extra))
    cfg.checkpoints.checkpoints_export_dir = str(tmp_path / "ckpt")
    cfg.base.tensorboard_export_dir = str(tmp_path / "tb")
    torch.manual_seed(0)
    return create_experiment("classification")(config=cfg, train_dataloader=[], valid_dataloader=SyntheticLoader(2, 16, seed=5, S=77, vocab_size=3000),
                                               test_dataloader=None, tokenizer=None)


def test_validate_fills_retrieval_and_returns_the_same_tuple(dev, tmp_path, monkeypatch):
    """One validate() of a tiny model with the shipped example selected: `self.retrieval` has the expected names and finite values;
    the same weights without the key return an equal 5-tuple and no retrieval."""
    with_key = _experiment(monkeypatch, tmp_path, ["+experiments/config/retrieval=recall", "experiments.config.retrieval.ks=[1,5]"])
    val = with_key.validate()
    torch.cuda.synchronize()
    names = {f"{d}_{k}" for d in ("i2t", "t2i") for k in ("R@1", "R@5", "median_rank", "mrr", "ties", "n_queries", "no_positive")}
    assert set(with_key.retrieval) == names and all(np.isfinite(v) for v in with_key.retrieval.values()), with_key.retrieval
    r = with_key.retrieval
    assert r["i2t_n_queries"] == r["t2i_n_queries"] == 32 and r["i2t_no_positive"] == 0
    assert 0.0 <= r["i2t_R@1"] <= r["i2t_R@5"] <= 1.0 and 1.0 <= r["t2i_median_rank"] <= 32.0 and 1.0 / 32 <= r["i2t_mrr"] <= 1.0
    without = _experiment(monkeypatch, tmp_path, [])
    without.model.load_state_dict(with_key.model.state_dict())
    val2 = without.validate()
    assert without.retrieval is None
    assert len(val) == 5 and np.isfinite(val[0]) and np.isfinite(val[1]) and val == val2, (val, val2)
