"""Exams as training samples, on the device: the view-pooling kernels (csrc/view_pool.hip) against torch, their documented corner rules, the
wiring tower -> pooling against the flat tower with torch pooling, the mean against the CPU oracle, and the whole model on batches of studies.

Bounds that are not the project's existing bars are derived, not measured:
  * max: a maximum of identical bits is exact -> bit equality (outputs, argmax, gradients);
  * mean: at most k - 1 sequential fp32 additions and one division, each with a relative rounding error <= 2^-24, of terms bounded by
    sum_v |f_v|: |out - ref| <= k 2^-23 sum_v |f_v| covers this kernel's order and whatever order torch sums in;
  * mean gradient: dout / k, one correctly rounded division on either side -> rtol 2^-22."""
import math
import os

import pytest
import torch

from oracle import encoders_oracle as E
from tests.conftest import measured

pytestmark = pytest.mark.gpu
CFG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmg-clip_amd", "configs")
NAN = float("nan")


def _rel(a, b):
    a, b = a.detach().float().cpu().double().flatten(), b.detach().float().cpu().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30)), float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))


def _randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if n.endswith("layer_scale"):
                p.copy_(0.3 + 0.7 * torch.rand(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "LayerNorm.weight" in n or (p.dim() == 1 and n.endswith("weight")):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() >= 2 and "embeddings" not in n:
                p.mul_(2.5)


def _counts(S, hi, seed):
    return torch.randint(1, hi + 1, (S,), generator=torch.Generator().manual_seed(seed)).tolist()


def _torch_pool(feat, counts, mode):
    """The reference's arithmetic per study: torch.stack(views).mean(0) / .max(0) -> (pooled [S, C], index of the winner inside the study)."""
    outs, idxs, o = [], [], 0
    for k in counts:
        stacked = torch.stack([feat[o + j] for j in range(k)])
        if mode == 0:
            outs.append(stacked.mean(0))
        else:
            m = stacked.max(0)
            outs.append(m[0])
            idxs.append(m[1] + o)
        o += k
    return torch.stack(outs), (torch.stack(idxs) if idxs else None)


def _mean_bound(feat, counts):
    o, rows = 0, []
    for k in counts:
        rows.append(k * 2.0 ** -23 * feat[o:o + k].abs().double().sum(0))
        o += k
    return torch.stack(rows)


def _run_kernels(feat, offs, S, V, C, mode, dout):
    """Both directions into buffers pre-filled with NaN."""
    from mmgclip import kernels as K
    dev = feat.device
    out = torch.full((S, C), NAN, device=dev)
    arg = torch.full((S, C), -7, device=dev, dtype=torch.int32) if mode == 1 else None
    got, gidx = K.view_pool_fwd(feat, offs, S, mode, out=out, argmax=arg)
    assert got.data_ptr() == out.data_ptr()
    dfeat = K.view_pool_bwd(dout, offs, gidx, V, mode, out=torch.full((V, C), NAN, device=dev))
    torch.cuda.synchronize()
    return got, gidx, dfeat


CASES = [(S, 4, C) for S in (1, 7, 64, 1000) for C in (8, 768, 1024, 2048)] + [(33, 9, 768), (5, 9, 3072)]


# ---- 1. kernels against torch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["mean", "max"])
@pytest.mark.parametrize("S,hi,C", CASES)
def test_view_pool_kernels_against_torch(dev, S, hi, C, mode):
    from mmgclip.networks.view_pool import study_offsets
    counts = _counts(S, hi, 100 + S + C)
    if hi == 9:
        counts[0] = 9
    V = sum(counts)
    g = torch.Generator().manual_seed(S * 7 + C)
    feat = torch.randn(V, C, generator=g)
    dout = torch.randn(S, C, generator=g)
    ref_in = feat.clone().requires_grad_(True)
    ref, ridx = _torch_pool(ref_in, counts, mode)
    ref.backward(dout)
    offs = study_offsets(counts).to(dev)
    got, gidx, dfeat = _run_kernels(feat.to(dev), offs, S, V, C, mode, dout.to(dev))
    assert not torch.isnan(got).any() and not torch.isnan(dfeat).any()          # every element written, nothing rests on a memset
    got_c, dfeat_c = got.cpu(), dfeat.cpu()
    if mode == 1:
        o = 0
        for k in counts:                                                        # continuous random data: no ties inside a study
            if k > 1:
                top = feat[o:o + k].topk(2, dim=0)[0]
                assert (top[0] > top[1]).all()
            o += k
        assert torch.equal(got_c, ref.detach())
        assert torch.equal(gidx.cpu().long(), ridx)
        assert torch.equal(dfeat_c, ref_in.grad)
    else:
        assert gidx is None
        err, bound = (got_c.double() - ref.detach().double()).abs(), _mean_bound(feat, counts)
        assert (err <= bound).all(), float((err - bound).max())
        torch.testing.assert_close(dfeat_c, ref_in.grad, rtol=2.0 ** -22, atol=0.0)
    again = _run_kernels(feat.to(dev), offs, S, V, C, mode, dout.to(dev))
    assert torch.equal(again[0], got) and torch.equal(again[2], dfeat) and (mode == 0 or torch.equal(again[1], gidx))


def test_view_pool_autograd_function(dev):
    """pool_views -> ViewPool: the same numbers through autograd, gradients for the features only, and what is saved."""
    from mmgclip.networks.view_pool import pool_views
    counts = [4, 1, 2, 3]
    feat = torch.randn(10, 768, generator=torch.Generator().manual_seed(1))
    wgt = torch.randn(4, 768, generator=torch.Generator().manual_seed(2))
    for method, mode in (("avg", 0), ("maxpool", 1)):
        a = feat.clone().to(dev).requires_grad_(True)
        out = pool_views(a, counts, method)
        saved = out.grad_fn.saved_tensors
        assert [t.dtype for t in saved] == [torch.int32] * (1 + mode) and saved[0].numel() == 5
        (out * wgt.to(dev)).sum().backward()
        b = feat.clone().requires_grad_(True)
        ref, _ = _torch_pool(b, counts, mode)
        (ref * wgt).sum().backward()
        if mode == 1:
            assert torch.equal(out.detach().cpu(), ref.detach()) and torch.equal(a.grad.cpu(), b.grad)
        else:
            assert ((out.detach().cpu().double() - ref.detach().double()).abs() <= _mean_bound(feat, counts)).all()
            torch.testing.assert_close(a.grad.cpu(), b.grad, rtol=2.0 ** -22, atol=0.0)
    stacked = pool_views(feat[:8].to(dev), [2, 2, 2, 2], "stack")
    assert stacked.shape == (4, 1536) and torch.equal(stacked[3].cpu(), torch.cat([feat[6], feat[7]]))


# ---- 2. documented corner rules ---------------------------------------------------------------------------------------------------------
def test_view_pool_tie_goes_to_the_lowest_row(dev):
    from mmgclip import kernels as K
    from mmgclip.networks.view_pool import study_offsets
    C = 8
    feat = torch.tensor([[0.0] * C, [1.0] * C, [5.0] * C, [5.0] * C, [2.0] * C, [5.0] * C], device=dev)      # study 1 = rows 1..5
    feat[3, 4:] = 6.0                                                        # columns 4..7: a single winner, row 3
    offs = study_offsets([1, 5]).to(dev)
    out, idx = K.view_pool_fwd(feat, offs, 2, 1)
    assert out[1].tolist() == [5.0] * 4 + [6.0] * 4 and idx[1].tolist() == [2] * 4 + [3] * 4 and idx[0].tolist() == [0] * C
    dout = torch.arange(1, 2 * C + 1, device=dev, dtype=torch.float32).reshape(2, C)
    dfeat = K.view_pool_bwd(dout, offs, idx, 6, 1)
    want = torch.zeros(6, C, device=dev)
    want[0] = dout[0]
    want[2, :4], want[3, 4:] = dout[1, :4], dout[1, 4:]
    assert torch.equal(dfeat, want)                                          # the whole gradient to the one recorded row


def test_view_pool_nan_view_gives_nan_and_its_row(dev):
    from mmgclip import kernels as K
    from mmgclip.networks.view_pool import study_offsets
    feat = torch.randn(7, 16, generator=torch.Generator().manual_seed(3)).to(dev)
    feat[4, 5] = NAN                                                         # study 1 = rows 3..6; a larger value follows the NaN
    feat[5, 5] = 100.0
    feat[0, 2] = NAN                                                         # the first row of study 0
    offs = study_offsets([3, 4]).to(dev)
    out, idx = K.view_pool_fwd(feat, offs, 2, 1)
    ref = torch.stack([feat[:3].max(0)[0], feat[3:].max(0)[0]])
    assert torch.isnan(out[1, 5]) and int(idx[1, 5]) == 4 and torch.isnan(out[0, 2]) and int(idx[0, 2]) == 0
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and int(torch.isnan(out).sum()) == 2
    keep = ~torch.isnan(ref)
    assert torch.equal(out[keep], ref[keep])
    mean, _ = K.view_pool_fwd(feat, offs, 2, 0)
    assert torch.isnan(mean[1, 5]) and torch.isnan(mean[0, 2]) and int(torch.isnan(mean).sum()) == 2


@pytest.mark.parametrize("mode", [0, 1])
def test_view_pool_of_single_views_is_the_identity(dev, mode):
    from mmgclip import kernels as K
    from mmgclip.networks.view_pool import study_offsets
    feat = torch.randn(9, 768, generator=torch.Generator().manual_seed(4)).to(dev)
    feat[2, :4] = torch.tensor([0.0, -0.0, float("inf"), 1e-42])
    offs = study_offsets([1] * 9).to(dev)
    out, idx = K.view_pool_fwd(feat, offs, 9, mode)
    assert torch.equal(out.view(torch.int32), feat.view(torch.int32))
    dfeat = K.view_pool_bwd(feat, offs, idx, 9, mode)
    assert torch.equal(dfeat.view(torch.int32), feat.view(torch.int32))
    if mode == 1:
        assert torch.equal(idx, torch.arange(9, device=dev, dtype=torch.int32)[:, None].expand(9, 768))


def test_view_pool_rejects_bad_arguments(dev):
    from mmgclip import _hip
    from mmgclip._hip import ptr, stream
    from mmgclip.networks.view_pool import study_offsets
    feat = torch.zeros(4, 6, device=dev)
    offs = study_offsets([2, 2]).to(dev)
    out, arg = torch.zeros(2, 6, device=dev), torch.zeros(2, 6, device=dev, dtype=torch.int32)
    lib = _hip.load()
    for mode in (0, 1):
        assert lib.mmg_view_pool_fwd(ptr(feat), ptr(offs), ptr(out), ptr(arg), 2, 6, mode, stream()) != 0           # C % 4
        assert "mmg_view_pool_fwd" in _hip.last_error()
        assert lib.mmg_view_pool_fwd(None, ptr(offs), ptr(out), ptr(arg), 2, 8, mode, stream()) != 0                # null feat
        assert "mmg_view_pool_fwd" in _hip.last_error()
        assert lib.mmg_view_pool_bwd(ptr(out), ptr(offs), ptr(arg), ptr(feat), 2, 4, 6, mode, stream()) != 0
        assert "mmg_view_pool_bwd" in _hip.last_error()
        assert lib.mmg_view_pool_bwd(None, ptr(offs), ptr(arg), ptr(feat), 2, 4, 8, mode, stream()) != 0
        assert "mmg_view_pool_bwd" in _hip.last_error()
    assert lib.mmg_view_pool_fwd(ptr(feat), ptr(offs), ptr(out), None, 2, 8, 1, stream()) != 0                      # max without argmax
    assert lib.mmg_view_pool_fwd(ptr(feat), ptr(offs), ptr(out), ptr(arg), 2, 8, 2, stream()) != 0                  # unknown mode
    assert lib.mmg_view_pool_fwd(ptr(feat), ptr(offs), ptr(out), ptr(arg), 0, 8, 0, stream()) != 0                  # no study
    assert lib.mmg_view_pool_fwd(ptr(feat), ptr(offs), ptr(out), ptr(arg), 2, 3076, 0, stream()) != 0               # C > 3072
    with pytest.raises(RuntimeError, match="mmg_view_pool_fwd"):
        _hip.call("mmg_view_pool_fwd", None, ptr(offs), ptr(out), ptr(arg), 2, 8, 0, stream())
    torch.cuda.synchronize()


# ---- 3. tower + pooling == flat tower + torch pooling -------------------------------------------------------------------------------------
STUDY_COUNTS = (4, 1, 2)
VIEW_SIZES = [(100, 70), (77, 50), (100, 70), (64, 64), (77, 50), (64, 64), (100, 70)]


def _views_and_weights():
    g = torch.Generator().manual_seed(2)
    views = [torch.rand(1, H, W, generator=g) for H, W in VIEW_SIZES]
    wgt = torch.randn(len(STUDY_COUNTS), 768, generator=torch.Generator().manual_seed(3))
    return views, wgt


def _nest(views):
    out, o = [], 0
    for k in STUDY_COUNTS:
        out.append(views[o:o + k])
        o += k
    return out


def _model_around(tower, method, dev):
    """MMGCLIP.encode_images needs `config`, `device` and `image_encoder` only: the method under test bound to a holder of those three."""
    from mmgclip.config import Config
    from mmgclip.networks.mmgclip_model import MMGCLIP

    class Holder:
        encode_images, _encode_studies, _view_method = MMGCLIP.encode_images, MMGCLIP._encode_studies, MMGCLIP._view_method
    h = Holder()
    h.config = Config.wrap({"networks": {"image_encoder": {"name": "ConvNextTinyEncoder", "image_features_dimension": 768}},
                            "dataset": {"config": {"n_images_per_study": 4, "concatenate_features_method": method}}})
    h.device, h.image_encoder = dev, tower
    return h


@pytest.mark.parametrize("checkpoint", [False, True], ids=["plain", "checkpoint"])
@pytest.mark.parametrize("method,mode", [("avgpool", 0), ("maxpool", 1)])
def test_tower_with_pooling_equals_flat_tower_with_torch_pooling(dev, method, mode, checkpoint):
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    torch.manual_seed(0)
    tower = ConvNextTinyEncoder(micro_batch=2, checkpoint=checkpoint)
    _randomize(tower, 1)
    tower = tower.to(dev)
    views, wgt = _views_and_weights()
    wgt = wgt.to(dev)
    # A: the nested batch through the model's new path
    pooled = _model_around(tower, method, dev).encode_images({"image": _nest(views)})
    assert pooled.shape == (3, 768)
    (pooled * wgt).sum().backward()
    grads_a = {n: p.grad.detach().clone() for n, p in tower.model.named_parameters()}
    tower.zero_grad(set_to_none=True)
    # B: the same seven views as a flat list through the tower, torch pooling on the device inside autograd
    f = tower([v.to(dev) for v in views])
    assert f.shape == (7, 768)
    ref, _ = _torch_pool(f, STUDY_COUNTS, mode)
    (ref * wgt).sum().backward()
    if mode == 1:
        assert torch.equal(pooled.detach(), ref.detach())
    else:
        err = (pooled.detach().double() - ref.detach().double()).abs().cpu()
        assert (err <= _mean_bound(f.detach().cpu(), STUDY_COUNTS)).all(), float(err.max())
    worst = max(_rel(grads_a[n], p.grad)[0] for n, p in tower.model.named_parameters())
    print("view pool wiring", method, "checkpoint", checkpoint, "grad rel max", worst)
    for n, p in tower.model.named_parameters():
        assert _rel(grads_a[n], p.grad)[0] < 2e-3, n


# ---- 4. mean mode, end to end against the oracle ---------------------------------------------------------------------------------------------
def test_mean_pooled_tower_against_the_oracle(dev):
    """Oracle: one convnext_forward per size group, gradients summed (as test_batch_of_images_of_different_sizes), torch mean per study on the
    CPU.  Bars of that test: features rel < 1.5e-2, cosine > 0.9999; every gradient cosine > 0.999, rel < 4e-2.  (Max is not compared with the
    oracle at gradient level: where two views' features lie closer than the tower's bf16 error the winner may legitimately differ.)"""
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    torch.manual_seed(0)
    tower = ConvNextTinyEncoder(micro_batch=2)
    _randomize(tower, 1)
    sd = {k[len("model."):]: v.clone() for k, v in tower.state_dict().items()}
    views, wgt = _views_and_weights()
    groups = {}
    for i, hw in enumerate(VIEW_SIZES):
        groups.setdefault(hw, []).append(i)
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    per_view = [None] * len(views)
    for hw, idx in groups.items():
        pooled, _ = E.convnext_forward(osd, torch.stack([views[i] for i in idx]), depths=(3, 3, 9, 3))
        for j, i in enumerate(idx):
            per_view[i] = pooled.flatten(1)[j]
    oref, _ = _torch_pool(per_view, STUDY_COUNTS, 0)
    (oref * wgt).sum().backward()                          # (one graph over all groups: the gradients are summed by autograd)
    tower = tower.to(dev)
    got = _model_around(tower, "avgpool", dev).encode_images({"image": _nest(views)})
    (got * wgt.to(dev)).sum().backward()
    fr, fc = _rel(got, oref)
    worst = {n: _rel(p.grad, osd[n].grad) for n, p in tower.model.named_parameters()}
    gr, gc = max(v[0] for v in worst.values()), min(v[1] for v in worst.values())
    print("view pool tower (mean) feat rel", fr, "cos", fc, "grad rel max", gr, "cos min", gc)
    measured("view_pool_tower", method="avgpool", studies=3, views=7, feat_rel=fr, feat_cos=fc, grad_rel_max=gr, grad_cos_min=gc)
    assert fr < 1.5e-2 and fc > 0.9999, (fr, fc)
    bad = {k: v for k, v in worst.items() if not (v[1] > 0.999 and v[0] < 4e-2)}
    assert not bad, f"{len(bad)} of {len(worst)} gradients off: {list(bad.items())[:8]}"


# ---- 5. whole model ---------------------------------------------------------------------------------------------------------------------------
def _small_bert(monkeypatch):
    from mmgclip.networks import bert
    orig = bert.BertConfigLite.__init__

    def small(self, **kw):
        kw.setdefault("num_hidden_layers", 2)
        kw.setdefault("vocab_size", 3000)
        orig(self, **kw)
    monkeypatch.setattr(bert.BertConfigLite, "__init__", small)


def _exam_cfg(tmp_path, extra=(), network="clip_convnexttiny_bert_pixels", batch=8):
    from mmgclip.config import compose
    return compose(CFG_DIR, "train_exam_reports_clf",
                   [f"networks={network}", "dataset=exam-reports-pixels", "tokenizer=bert_clinical_seqlen=77", "networks/dropout=dropout0",
                    "networks.image_encoder.micro_batch=4", "scheduler=warmup1_epo15", "optimizer.config.learning_rate=1e-3",
                    f"dataloader.train.batch_size={batch}", "dataset.config.synthetic_samples=12",
                    f"checkpoints.checkpoints_export_dir={tmp_path}/ckpt", f"base.tensorboard_export_dir={tmp_path}/tb", *extra])


@pytest.mark.parametrize("method", ["avgpool", "maxpool"])
def test_whole_model_trains_on_exams(dev, tmp_path, monkeypatch, method):
    """train_exam_reports_clf + ConvNeXt-T pixels + dataset=exam-reports-pixels (small BERT, default initialisation): one ClassifierExperiment.train
    epoch on the loader train.py builds - batches of 8 exams of 1..4 views of three sizes.  The loss is finite and within 0.5 of ln(8), every
    trainable parameter has a finite gradient, non-zero except BERT's unused pooler, and moved (the bars of
    test_whole_model_trains_at_a_rectangular_native_size_and_on_mixed_sizes)."""
    import train
    from mmgclip.dataset.synthetic import SyntheticLoader
    from mmgclip.experiments.experiments_controller import create_experiment
    _small_bert(monkeypatch)
    batch = 8
    cfg = _exam_cfg(tmp_path, [f"dataset.config.concatenate_features_method={method}"])
    loaders = train.build_loaders(cfg)
    assert loaders[0].kw["views_per_study"] == (1, 4)
    loader = SyntheticLoader(1, batch, seed=5, **{**loaders[0].kw, "vocab_size": 3000})
    first = next(iter(loader))
    counts = [len(s) for s in first["image"]]
    assert len(first["image"]) == batch and max(counts) > 1 and len({tuple(v.shape) for s in first["image"] for v in s}) > 1
    torch.manual_seed(0)
    exp = create_experiment(cfg.experiments.config.experiment_name)(config=cfg, train_dataloader=loader, valid_dataloader=None,
                                                                    test_dataloader=None, tokenizer=None)
    exp.scheduler.step()                                   # (the first epoch of the warm-up schedule runs at lr = 0: take the second one's rate)
    assert exp.optimizer.param_groups[0]["lr"] > 0
    before = {n: p.detach().clone() for n, p in exp.model.named_parameters() if p.requires_grad}
    loss = exp.train()
    print("exam epoch", method, "loss", loss, "views per study", counts)
    assert math.isfinite(loss) and abs(loss - math.log(batch)) < 0.5, loss
    bad = [n for n, p in exp.model.named_parameters() if p.requires_grad and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not bad, bad[:5]
    dead = [n for n, p in exp.model.named_parameters() if p.requires_grad and not p.grad.any()]
    assert all(".pooler." in n for n in dead), dead[:5]
    still = [n for n, p in exp.model.named_parameters() if p.requires_grad and n not in dead and torch.equal(p.detach(), before[n])]
    assert not still, still[:5]
    # validation goes through the same model call: a batch of exams gives one row of similarities per exam
    exp.valid_dataloader = [next(iter(SyntheticLoader(1, batch, seed=9, **{**loaders[1].kw, "vocab_size": 3000})))]
    val = exp.validate()
    assert math.isfinite(val[0])


def test_whole_model_on_exams_of_one_view_equals_the_flat_batch_and_other_forms(dev, tmp_path, monkeypatch):
    from mmgclip.dataset.synthetic import synthetic_batch
    from mmgclip.evaluator import Evaluator
    from mmgclip.networks.mmgclip_model import MMGCLIP
    _small_bert(monkeypatch)
    n = 4
    for method in ("avgpool", "maxpool"):
        torch.manual_seed(0)
        model = MMGCLIP(_exam_cfg(tmp_path, [f"dataset.config.concatenate_features_method={method}"])).train()
        flat = synthetic_batch(n, S=77, image_size=(77, 50), vocab_size=3000, seed=6)
        ref = model(dict(flat), materialize_logits=False)["image_embeddings"].detach().clone()
        nested = dict(flat)
        nested["image"] = [[flat["image"][i]] for i in range(n)]
        got = model(nested, materialize_logits=False)["image_embeddings"].detach()
        assert got.shape == (n, 512) and torch.equal(got, ref), method
        # the same through a list of images of two sizes
        other = torch.rand(n, 1, 64, 64, generator=torch.Generator().manual_seed(7))
        mixed = [flat["image"][i] if i % 2 == 0 else other[i] for i in range(n)]
        ref = model({**flat, "image": mixed}, materialize_logits=False)["image_embeddings"].detach().clone()
        got = model({**flat, "image": [(v,) for v in mixed]}, materialize_logits=False)["image_embeddings"].detach()
        assert torch.equal(got, ref), method
    # Evaluator.encode_image on a batch of exams: one embedding per exam
    exams = synthetic_batch(5, S=77, vocab_size=3000, seed=8, views_per_study=(1, 4), view_sizes=[(100, 70), (77, 50)])
    emb = Evaluator(model.config, model=model).encode_image(exams, as_numpy=False)
    assert emb.shape == (5, 512) and torch.isfinite(emb).all()
    model.train()
    # a 5-D tensor [S, k, Cin, H, W] is the same batch as the nested list of its views
    five = torch.rand(3, 2, 1, 64, 64, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        a = model.encode_images({"image": five})
        b = model.encode_images({"image": [[five[s, j] for j in range(2)] for s in range(3)]})
    assert a.shape == (3, 768) and torch.equal(a, b)
    # more views than dataset.config.n_images_per_study: the dataset's job, an error here
    with pytest.raises(ValueError, match="n_images_per_study"):
        model.encode_images({"image": [[five[0, 0]] * 5]})
    with pytest.raises(ValueError, match="list of non-empty lists"):
        model.encode_images({"image": [[five[0, 0]], []]})


def test_whole_model_stack_needs_k_times_the_feature_dimension(dev, tmp_path, monkeypatch):
    from mmgclip.dataset.synthetic import synthetic_batch
    from mmgclip.loss.loss_controller import create_loss
    from mmgclip.networks.mmgclip_model import MMGCLIP
    _small_bert(monkeypatch)
    batch = synthetic_batch(4, S=77, vocab_size=3000, seed=3, views_per_study=(2, 2), view_sizes=[(64, 64), (77, 50)])
    torch.manual_seed(0)
    model = MMGCLIP(_exam_cfg(tmp_path, ["dataset.config.concatenate_features_method=stack",
                                         "networks.image_encoder.image_features_dimension=1536"])).train()
    assert model.image_projection_layer is not None
    out = model(dict(batch), materialize_logits=False)
    assert out["image_embeddings"].shape == (4, 512)
    loss, _ = create_loss("CLIPLoss")()(**out)
    loss.backward()
    model.join_streams()
    torch.cuda.synchronize()
    assert math.isfinite(loss.item())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.image_encoder.parameters() if p.requires_grad)
    ragged = synthetic_batch(4, S=77, vocab_size=3000, seed=3, views_per_study=(1, 2), view_sizes=[(64, 64)])
    assert len({len(s) for s in ragged["image"]}) == 2
    with pytest.raises(ValueError, match="same number of views"):
        model.encode_images(ragged)
    torch.manual_seed(0)
    narrow = MMGCLIP(_exam_cfg(tmp_path, ["dataset.config.concatenate_features_method=stack"])).train()
    with pytest.raises(ValueError, match="image_features_dimension=1536"):
        narrow(dict(batch), materialize_logits=False)


# ---- 6. ViT -------------------------------------------------------------------------------------------------------------------------------------
def test_vit_takes_exams_of_equal_sized_views_only(dev, tmp_path, monkeypatch):
    from mmgclip.networks.mmgclip_model import MMGCLIP
    _small_bert(monkeypatch)
    torch.manual_seed(0)
    model = MMGCLIP(_exam_cfg(tmp_path, ["networks.image_encoder.image_size=64", "dataset.config.concatenate_features_method=maxpool"],
                              network="clip_vitb16_bert_pixels")).train()
    five = torch.rand(3, 2, 1, 64, 64, generator=torch.Generator().manual_seed(1))
    feat = model.encode_images({"image": five})
    assert feat.shape == (3, model.image_encoder.model_output_dimension) and torch.isfinite(feat).all()
    feat.sum().backward()
    grads = [p.grad for p in model.image_encoder.parameters() if p.requires_grad]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
    nested = model.encode_images({"image": [[five[s, 0], five[s, 1]] for s in range(3)]})
    assert torch.equal(nested.detach(), feat.detach())
    with pytest.raises(ValueError, match="every view"):
        model.encode_images({"image": [[five[0, 0], torch.rand(1, 48, 48)], [five[1, 0]]]})
