"""The sigmoid pairwise loss on the MI355X: the kernels of csrc/sigmoid_head.hip through `_hip.call` on the test's own buffers, then
`SigmoidCLIPLoss` and the model, against the float64 reference and the derived bars of tests/sigmoid_ref.py.

Every kernel call writes into buffers pre-filled with NaN bits (dscale / dbias, which accumulate, with 0.5 and -3) and followed by 32
sentinel entries or rows; no output may keep a NaN and no sentinel may change.

Shapes (n_loc, N, D, diag_off): sigmoid_ref.SHAPES - one pair; a partial tile; a tile and one more; three row tiles at the widest D;
c + 1 columns with c = 128 the columns one workgroup pass covers (4 waves x 32; restated as sigmoid_ref.COLS_PER_PASS); rows of a rank
that is not the first; and (64, 128, 512) twice as two simulated ranks.  Both positives modes; the cluster mode on hand-made labels with
a cluster across the tile seam and a singleton.  gout NULL and 0.25; dscale / dbias NULL and given.

Exact regime (torch.equal): one-hot rows, s = 256, b = -128, coef and gout powers of two (coef is an argument of the kernel: 1/N
where N is a power of two, the next power of two's reciprocal otherwise).  The preconditions are asserted on the reference alone
(sigmoid_ref.exactness_violations; also tests/test_sigmoid_ref_cpu.py).
Gaussian regime: random unit rows, (s, b) in sigmoid_ref.SB_PAIRS, outputs inside the derived bars; the worst ratios are recorded
through conftest.measured (committed copy: profiles/sigmoid_measured_tolerances.jsonl)."""
import functools
import math
import os

import pytest
import torch

from tests import sigmoid_ref as R
from tests.conftest import measured

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "mmg-clip_amd", "configs")
TAIL = 32
SENTINEL = 12345.0
NAN_BITS = 0x7FC00ABC
DS0, DB0 = 0.5, -3.0


def _out(dev, rows, cols=None, fill=None):
    """rows (+ TAIL sentinel rows) of NaN bits, or of `fill` for an accumulated scalar."""
    shape = (rows + TAIL,) if cols is None else (rows + TAIL, cols)
    t = torch.full(shape, SENTINEL, device=dev, dtype=torch.float32)
    if fill is None:
        t[:rows].view(torch.int32).fill_(NAN_BITS)
    else:
        t[:rows] = fill
    return t


def _take(t, rows):
    assert bool((t[rows:] == SENTINEL).all()), "a sentinel after the output changed"
    out = t[:rows].cpu()
    assert not bool(torch.isnan(out).any()), "an owned element kept its NaN fill (or the kernel produced one)"
    return out


def _launch(dev, X, Y, s, b, key, lab, off, coef, gout, scalars=True):
    """One forward and one backward launch on fresh buffers -> row_loss, dX, dscale, dbias (CPU; the scalars None when not asked for)."""
    from mmgclip._hip import call, ptr, stream
    n, D = X.shape
    N = Y.shape[0]
    Xd, Yd = X.to(dev).contiguous(), Y.to(dev).contiguous()
    sd, bd = torch.tensor([s], device=dev, dtype=torch.float32), torch.tensor([b], device=dev, dtype=torch.float32)
    kd = None if key is None else key.to(dev).contiguous()
    ld = None if lab is None else lab.to(dev).contiguous()
    gd = None if gout is None else torch.tensor([gout], device=dev, dtype=torch.float32)
    row_loss, dX = _out(dev, n), _out(dev, n, D)
    ds = _out(dev, 1, fill=DS0) if scalars in (True, "dscale") else None          # scalars: True (both), False (both NULL), or one name
    db = _out(dev, 1, fill=DB0) if scalars in (True, "dbias") else None
    call("mmg_sigmoid_rows_fwd", ptr(Xd), ptr(Yd), ptr(sd), ptr(bd), ptr(kd), ptr(ld), n, N, D, off, ptr(row_loss), stream())
    call("mmg_sigmoid_rows_bwd", ptr(Xd), ptr(Yd), ptr(sd), ptr(bd), ptr(kd), ptr(ld), ptr(gd), coef, n, N, D, off, ptr(dX), ptr(ds),
         ptr(db), stream())
    torch.cuda.synchronize()
    return (_take(row_loss, n), _take(dX, n), None if ds is None else _take(ds, 1)[0], None if db is None else _take(db, 1)[0])


@functools.lru_cache(maxsize=None)
def _gauss(shape, mode, sb, gout):
    """Inputs and the float64 reference of one Gaussian case, computed once and shared (read-only)."""
    n, N, D, off = shape
    X, Y = R.gaussian_case(n, N, D, seed=7 * N + D)
    key, lab = R.keys_for(mode, n, N, off)
    s, b, coef = R.f32(sb[0]), R.f32(sb[1]), R.f32(1.0 / N)
    ref = R.reference(X, Y, s, b, R.positive_mask(n, N, off, key, lab), coef, 1.0 if gout is None else gout, DS0, DB0)
    return X, Y, key, lab, s, b, coef, ref


def _ratios(ref, got):
    row_loss, dX, ds, db = got
    q = dict(row_loss=R.ratio(row_loss, ref.row_loss, ref.E_row_loss), dX=R.ratio(dX, ref.dX, ref.E_dX))
    if ds is not None:
        q.update(dscale=R.ratio(ds, ref.dscale, ref.E_dscale), dbias=R.ratio(db, ref.dbias, ref.E_dbias))
    return q


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_gaussian_regime_inside_the_bars(dev, shape, mode):
    worst = {}
    for k, sb in enumerate(R.SB_PAIRS):
        for gout in (None, 0.25):
            X, Y, key, lab, s, b, coef, ref = _gauss(shape, mode, sb, gout)
            scalars = not (k == 1 and gout is None)             # one combination runs with dscale = dbias = NULL
            q = _ratios(ref, _launch(dev, X, Y, s, b, key, lab, shape[3], coef, gout, scalars))
            print(shape, mode, sb, gout, q)
            for name, v in q.items():
                worst[name] = max(worst.get(name, 0.0), v)
    measured("sigmoid_gaussian", shape=str(shape), mode=mode, k_fn=R.K_FN, **worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_exact_regime_is_bit_exact(dev, shape, mode):
    n, N, D, off = shape
    coef = 2.0 ** -math.ceil(math.log2(N))
    X, Y, key, lab = R.exact_case(n, N, D, off, mode == "clusters")
    pos = R.positive_mask(n, N, off, key, lab)
    for gout in (None, 0.25):
        ref = R.reference(X, Y, R.EXACT_S, R.EXACT_B, pos, coef, 1.0 if gout is None else gout, DS0, DB0)
        assert R.exactness_violations(ref, pos, coef, 1.0 if gout is None else gout, DS0, DB0) == []
        row_loss, dX, ds, db = _launch(dev, X, Y, R.EXACT_S, R.EXACT_B, key, lab, off, coef, gout)
        assert torch.equal(row_loss, ref.row_loss.float())
        assert torch.equal(dX, ref.dX.float())
        assert float(ds) == float(ref.dscale) and float(db) == float(ref.dbias), (float(ds), float(ref.dscale), float(db), float(ref.dbias))
    want_dX, want_ds, want_db = (ref.dX / 0.25).float(), DS0 + (float(ref.dscale) - DS0) / 0.25, DB0 + (float(ref.dbias) - DB0) / 0.25
    for scalars in (False, "dscale", "dbias"):                      # either scalar may be NULL on its own; gout NULL = 1
        row_loss, dX, ds, db = _launch(dev, X, Y, R.EXACT_S, R.EXACT_B, key, lab, off, coef, None, scalars=scalars)
        assert torch.equal(row_loss, ref.row_loss.float()) and torch.equal(dX, want_dX)
        assert (ds is None) == (scalars != "dscale") and (db is None) == (scalars != "dbias")
        assert (ds is None or float(ds) == want_ds) and (db is None or float(db) == want_db)


@pytest.mark.parametrize("mode", R.MODES)
def test_two_simulated_ranks_equal_one_launch_and_the_unsharded_reference(dev, mode):
    """(64, 128, 512) twice: rank r holds rows 64 r .. 64 r + 63 of the 128.  A row's results do not depend on the rows around it, so
    row_loss and dX are those of one launch at n_loc = 128 bit for bit; the scalars are the sum over ranks, inside the bars."""
    N, D, nl = 128, 512, 64
    X, Y = R.gaussian_case(N, N, D, seed=11)
    lab = None if mode == "diagonal" else R.hand_labels(N)
    s, b, coef = R.f32(10.0), R.f32(-10.0), R.f32(1.0 / N)
    ref = R.reference(X, Y, s, b, R.positive_mask(N, N, 0, lab, lab), coef, 0.25, 2 * DS0, 2 * DB0, ranks=2)
    parts = [_launch(dev, X[r * nl:(r + 1) * nl], Y, s, b, None if lab is None else lab[r * nl:(r + 1) * nl], lab, r * nl, coef, 0.25)
             for r in range(2)]
    one = _launch(dev, X, Y, s, b, lab, lab, 0, coef, 0.25)
    row_loss, dX = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    assert torch.equal(row_loss, one[0]) and torch.equal(dX, one[1])
    q = _ratios(ref, (row_loss, dX, parts[0][2] + parts[1][2], parts[0][3] + parts[1][3]))
    print(mode, q)
    measured("sigmoid_two_ranks", mode=mode, k_fn=R.K_FN, **q)
    assert max(q.values()) <= 1.0, q


def test_row_loss_and_dx_are_bit_identical_over_three_runs(dev):
    X, Y, key, lab, s, b, coef, _ = _gauss((32, R.COLS_PER_PASS + 1, 512, 0), "clusters", R.SB_PAIRS[0], 0.25)
    runs = [_launch(dev, X, Y, s, b, key, lab, 0, coef, 0.25) for _ in range(3)]
    assert all(torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]) for r in runs[1:])


@pytest.mark.parametrize("mode", R.MODES)
def test_loss_class_through_l2normalize_scale_and_bias(dev, mode):
    """SigmoidCLIPLoss on un-normalised leaves: loss, d/d normalised embeddings, d/d exp-scale and d/d bias against the reference taken
    from the device's own normalised fp32 rows (the bars apply as derived); the leaf gradients through L2Normalize's backward
    dx = (dy - y <y,dy>) / norm with the bar of dy carried through it plus (Kd(D) + 8) u on its own arithmetic."""
    from mmgclip import head
    from mmgclip.loss.loss_controller import create_loss
    from tests.test_averaged_fused_cpu import THRESHOLD, assert_threshold_margin, clustered_inputs
    N, D = 72, 64
    img, txt = clustered_inputs(N, D, 7, seed=1)
    assert_threshold_margin(txt)
    a, t = img.to(dev).requires_grad_(True), txt.to(dev).requires_grad_(True)
    ls = torch.tensor(math.log(10.0), device=dev, requires_grad=True)
    bias = torch.tensor(-10.0, device=dev, requires_grad=True)
    ie, te = head.L2Normalize.apply(a), head.L2Normalize.apply(t)
    ie.retain_grad()
    te.retain_grad()
    scale = ls.exp()
    scale.retain_grad()
    crit = create_loss("SigmoidCLIPLoss")(positives=mode, similarity_threshold=THRESHOLD)
    loss, labels = crit(image_embeddings=ie, text_embeddings=te, logit_scale=scale, logit_bias=bias)
    loss.backward()
    torch.cuda.synchronize()
    e = torch.nn.functional.normalize(txt.double(), dim=1)
    from oracle import clip_oracle as O
    want_labels = torch.tensor(O.assign_labels(e @ e.t(), THRESHOLD), dtype=torch.int64)
    assert labels.cpu().tolist() == (list(range(N)) if mode == "diagonal" else want_labels.tolist()) and not labels.requires_grad
    ref = R.reference_loss(ie.detach().cpu(), te.detach().cpu(), float(scale.detach()), float(bias.detach()),
                           None if mode == "diagonal" else want_labels)
    q = dict(loss=R.ratio(loss.detach().cpu(), ref.loss, ref.E_loss), dimg=R.ratio(ie.grad.cpu(), ref.dimg, ref.E_dimg),
             dtxt=R.ratio(te.grad.cpu(), ref.dtxt, ref.E_dtxt), dscale=R.ratio(scale.grad.cpu(), ref.dscale, ref.E_dscale),
             dbias=R.ratio(bias.grad.cpu(), ref.dbias, ref.E_dbias))
    sv = float(scale.detach())
    q["dlogit_scale"] = R.ratio(ls.grad.cpu(), ref.dscale * sv, ref.E_dscale * sv + 2 * R.U * abs(float(ref.dscale) * sv))
    for name, leaf, y, dy, E in (("da", img, ie, ref.dimg, ref.E_dimg), ("dt", txt, te, ref.dtxt, ref.E_dtxt)):
        y = y.detach().cpu().double()
        norm = leaf.double().norm(dim=1, keepdim=True)
        want = (dy - y * (y * dy).sum(1, keepdim=True)) / norm
        bar = (E + y.abs() * (y.abs() * E).sum(1, keepdim=True)) / norm \
            + (R.Kd(D) + 8) * R.U * (dy.abs() + y.abs() * (y * dy).abs().sum(1, keepdim=True)) / norm
        q[name] = R.ratio((a if name == "da" else t).grad.cpu(), want, bar)
    print(mode, q)
    measured("sigmoid_loss_class", mode=mode, k_fn=R.K_FN, **q)
    assert max(q.values()) <= 1.0, q


def _small_model(monkeypatch, loss, extra=()):
    from mmgclip.config import compose
    from mmgclip.networks import bert
    from mmgclip.networks.mmgclip_model import MMGCLIP
    orig = bert.BertConfigLite.__init__

    def small(self, **kw):
        kw.setdefault("num_hidden_layers", 2)
        kw.setdefault("vocab_size", 3000)
        orig(self, **kw)
    monkeypatch.setattr(bert.BertConfigLite, "__init__", small)
    torch.manual_seed(0)
    cfg = compose(CFG_DIR, "train_binary_class_clf", ["networks.text_encoder.random_init=true", "tokenizer=bert_clinical_seqlen=77",
                                                      f"loss={loss}"] + list(extra))
    return cfg, MMGCLIP(cfg).train()


@pytest.mark.parametrize("learnable", [True, False])
def test_one_optimizer_step_moves_the_bias_and_a_learnable_scale(dev, monkeypatch, learnable):
    """MMGCLIP at the small test config with loss=sigmoid, one FusedAdamW step over the no-decay groups: logit_bias moves, logit_scale
    moves when it is a parameter, and the state dict (what EarlyStopper checkpoints) carries the bias."""
    from mmgclip.dataset.synthetic import synthetic_batch
    from mmgclip.loss.loss_controller import create_loss
    from mmgclip.optim import FusedAdamW
    from mmgclip.optim_groups import build_param_groups
    cfg, model = _small_model(monkeypatch, "sigmoid", ["networks.learnable_logit_scale=true", "networks.logit_temperature=0.1"] if learnable else [])
    assert float(model.logit_bias.detach()) == -10.0 and isinstance(model.logit_scale, torch.nn.Parameter) == learnable
    crit = create_loss(cfg.loss.config.loss_name)(positives=cfg.loss.config.positives)
    opt = FusedAdamW(build_param_groups(model, 1e-2, 0.05, no_decay_1d=True), lr=1e-2, weight_decay=0.05)
    out = model(synthetic_batch(8, S=77, vocab_size=3000, seed=4), materialize_logits=False)
    assert out["logit_bias"] is model.logit_bias and "logits_per_image" not in out
    s0 = float(model.logit_scale.detach())
    loss, labels = crit(**out)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and labels.tolist() == list(range(8))
    assert model.logit_bias.grad is not None and float(model.logit_bias.grad) != 0.0
    assert abs(float(model.logit_bias.detach()) + 10.0) == pytest.approx(1e-2, rel=1e-3)            # the first Adam step is lr, no decay
    assert (float(model.logit_scale.detach()) != s0) == learnable
    assert "logit_bias" in model.state_dict() and ("logit_scale" in model.state_dict()) == learnable


def test_clip_model_step_launches_what_it_launched_before(dev, monkeypatch):
    """loss=clip: no bias anywhere, and the head's launches of one step are the nine of the fused CLIP loss, in their order."""
    from mmgclip import head
    from mmgclip.dataset.synthetic import synthetic_batch
    from mmgclip.loss.loss_controller import create_loss
    cfg, model = _small_model(monkeypatch, "clip")
    seen = []

    def spy(name, *args, _call=head.call):
        seen.append(name)
        return _call(name, *args)
    monkeypatch.setattr(head, "call", spy)
    out = model(synthetic_batch(8, S=77, vocab_size=3000, seed=4), materialize_logits=False)
    loss, _ = create_loss("CLIPLoss")()(**out)
    loss.backward()
    torch.cuda.synchronize()
    assert "logit_bias" not in out and not hasattr(model, "logit_bias") and "logit_bias" not in model.state_dict()
    assert seen == ["mmg_l2norm_fwd"] * 2 + ["mmg_clip_rows_fwd"] * 2 + ["mmg_clip_loss_reduce"] + ["mmg_clip_rows_bwd_fused"] * 2 \
        + ["mmg_l2norm_bwd"] * 2, seen
