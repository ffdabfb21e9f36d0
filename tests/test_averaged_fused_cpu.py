"""AveragedMedicalCLIPLoss on the global batch, CPU side: the collective choreography of `head.FusedAveragedLoss` over gloo with
world sizes 2 and 4.  The device arithmetic (`head._HipAveragedBackend`) is replaced, inside the worker processes only, by the torch
restatement below; Comm, GradSync and the autograd Function are the product code.  Loss, text gradient, the tiny tower's weight
gradient after `GradSync.finish()` and d loss / d logit_scale must equal the unsharded float64 oracle
(`oracle.clip_oracle.averaged_medical_clip_loss` and its autograd) on every rank to 1e-5 relative (fp32 restatement against float64:
rounding is ~1e-7 per operation), and the labels a rank gets back are the global cluster ids of its rows."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLD = 0.65


def _paths():
    for p in (ROOT, os.path.join(ROOT, "mmg-clip_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


class TorchAveragedBackend:
    """`head._HipAveragedBackend` in plain torch, in the dtype of its operands."""

    @staticmethod
    def cluster(txt_all, threshold):
        from oracle import clip_oracle as O
        e = torch.nn.functional.normalize(txt_all.detach(), dim=1)
        lab = O.assign_labels(e @ e.t(), threshold)
        labels = torch.tensor(lab, dtype=torch.int64)
        return labels, torch.bincount(labels, minlength=len(lab)).to(torch.int32), max(lab) + 1

    @staticmethod
    def centroids(txt_all, labels, k):
        return torch.stack([txt_all[labels == c].mean(dim=0) for c in range(k)])

    @staticmethod
    def rows_forward(x_loc, y, scale, row_label):
        z = scale * (x_loc @ y.t())
        return torch.logsumexp(z, dim=1), z[torch.arange(x_loc.shape[0]), row_label]

    @staticmethod
    def loss_sum(lse_i, pos_i, lse_t, pos_t, coef):
        return (coef * ((lse_i - pos_i).sum() + (lse_t - pos_t).sum())).reshape(1)

    @staticmethod
    def rows_backward_row(x_loc, y, scale, lse_row, row_label, gout, coef, dx, dscale):
        zz = x_loc @ y.t()
        g = torch.exp(scale * zz - lse_row[:, None])
        g[torch.arange(x_loc.shape[0]), row_label] -= 1.0
        g = g * (coef * gout)
        if dscale is not None:
            dscale += (g * zz).sum()
        d = scale * (g @ y)
        return d if dx is None else dx.add_(d)

    @staticmethod
    def rows_backward_col(x_loc, y, scale, lse_col, col_label, row_key, key_off, counts, gout, coef, dx):
        key = row_key if row_key is not None else key_off + torch.arange(x_loc.shape[0])
        g = torch.exp(scale * (x_loc @ y.t()) - lse_col[None, :]) - (col_label[None, :] == key[:, None]).to(x_loc.dtype)
        w = torch.ones(x_loc.shape[0], dtype=x_loc.dtype) if counts is None else 1.0 / counts[key].to(x_loc.dtype)
        d = scale * ((g * (coef * gout * w)[:, None]) @ y)
        return d if dx is None else dx.add_(d)


def clustered_inputs(N, D, groups, seed):
    """Images random; text rows normalize(prototype[g] + 0.05 noise): reports of one prototype are far above the threshold, reports
    of different prototypes far below it, so the clustering cannot flip between fp32 and float64.  Every prototype is used.
    The noise is 0.05 per element at D = 64 and keeps that NORM (0.4 of the unit prototype) at every other D: at a fixed 0.05 per
    element its norm grows with sqrt(D) and at D = 160 the same-prototype cosines would sit on the threshold."""
    g = torch.Generator().manual_seed(seed)
    protos = torch.nn.functional.normalize(torch.randn(groups, D, generator=g), dim=1)
    member = (torch.arange(N) % groups)[torch.randperm(N, generator=g)]
    txt = torch.nn.functional.normalize(protos[member] + 0.05 * (64.0 / D) ** 0.5 * torch.randn(N, D, generator=g), dim=1)
    img = torch.randn(N, D, generator=g)
    return img, txt * (1.0 + torch.rand(N, 1, generator=g))         # un-normalised leaves: L2Normalize is in the chain


def assert_threshold_margin(txt, threshold=THRESHOLD, margin=1e-3):
    """A condition on the INPUTS (float64, host): no off-diagonal cosine within `margin` of the clustering threshold."""
    e = torch.nn.functional.normalize(txt.double(), dim=1)
    cos = e @ e.t()
    off = cos[~torch.eye(cos.shape[0], dtype=torch.bool)]
    gap = float((off - threshold).abs().min())
    assert gap > margin, gap
    return gap


def oracle_unsharded(img, txt, ls_param, threshold=THRESHOLD):
    """float64: oracle loss, labels and gradients w.r.t. the un-normalised leaves and the logit-scale parameter."""
    from oracle import clip_oracle as O
    a, b = img.double().clone().requires_grad_(True), txt.double().clone().requires_grad_(True)
    s = ls_param.double().clone().requires_grad_(True)
    loss, labels = O.averaged_medical_clip_loss(**O.forward_tail(a, b, s), similarity_threshold=threshold)
    loss.backward()
    return loss.detach(), labels, a.grad, b.grad, s.grad


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    _paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from mmgclip import distributed, head
    from oracle import clip_oracle as O
    comm = distributed.init_from_env("gloo")
    N, D = 72, 64
    img_all, txt_all = clustered_inputs(N, D, 7, seed=1)
    gap = assert_threshold_margin(txt_all)
    nl = N // world
    sl = slice(rank * nl, (rank + 1) * nl)
    torch.manual_seed(0)          # a tiny trainable "tower" on the image side: shared weights, different data per rank
    w_img = torch.nn.Parameter(torch.eye(D) + 0.01 * torch.randn(D, D))
    ls = torch.nn.Parameter(torch.tensor(float(np.log(1 / 0.07))))
    txt = txt_all[sl].clone().requires_grad_(True)
    head._HipAveragedBackend = TorchAveragedBackend          # this worker process only
    loss, labels = head.fused_averaged_loss(O.l2_normalize(img_all[sl] @ w_img.t()), O.l2_normalize(txt), ls.exp(), THRESHOLD, comm)
    loss.backward()
    distributed.GradSync(comm, arenas=(), extra_params=[w_img, ls]).finish()
    # unsharded float64 oracle on every rank (the tower's weight gradient through the same product)
    w2 = w_img.detach().double().requires_grad_(True)
    t2 = txt_all.double().clone().requires_grad_(True)
    ls2 = ls.detach().double().requires_grad_(True)
    ref, ref_labels = O.averaged_medical_clip_loss(**O.forward_tail(img_all.double() @ w2.t(), t2, ls2), similarity_threshold=THRESHOLD)
    ref.backward()
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())      # noqa: E731
    q.put(dict(rank=rank, gap=gap, k=int(ref_labels.max()) + 1, loss=rel(loss.detach().reshape(1), ref.detach().reshape(1)),
               dw=rel(w_img.grad, w2.grad), dls=rel(ls.grad.reshape(1), ls2.grad.reshape(1)), dtxt=rel(txt.grad, t2.grad[sl]),
               labels_ok=labels.tolist() == ref_labels[sl].tolist(), calls=comm.report()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_global_batch_averaged_loss_and_grad_sync_gloo(world):
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
    for r in results:
        assert r["k"] == 7 and r["labels_ok"], r                       # the global cluster ids of the rank's own rows
        assert r["loss"] < 1e-5 and r["dtxt"] < 1e-5 and r["dw"] < 1e-5 and r["dls"] < 1e-5, r
        c = r["calls"]                                                  # the exchanges are FusedClipLoss's: 4 gathers, the loss, the grads
        assert c["all_gather_calls"] == 4 and c["all_reduce_calls"] == 2, c
        assert c["all_gather_bytes"] == 2 * (72 * 64 * 4) + 2 * (72 * 4), c


def test_restated_backend_matches_the_oracle_unsharded():
    """comm=None, float32 restatement against the float64 oracle: the arithmetic of DESIGN.md §6 (centroids by linearity,
    ROW / COL products, dscale from the ROW products only) at N = 72, D = 64, seven clusters."""
    _paths()
    from mmgclip import head
    from oracle import clip_oracle as O
    img, txt = clustered_inputs(72, 64, 7, seed=1)
    assert_threshold_margin(txt)
    ls = torch.tensor(float(np.log(1 / 0.07)))
    ref, ref_labels, dimg, dtxt, dls = oracle_unsharded(img, txt, ls)
    a, b, s = img.clone().requires_grad_(True), txt.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    orig, head._HipAveragedBackend = head._HipAveragedBackend, TorchAveragedBackend
    try:
        loss, labels = head.fused_averaged_loss(O.l2_normalize(a), O.l2_normalize(b), s.exp(), THRESHOLD, None)
        loss.backward()
    finally:
        head._HipAveragedBackend = orig
    assert labels.tolist() == ref_labels.tolist() and not labels.requires_grad
    assert abs(float(loss.detach()) - float(ref)) < 1e-5 * abs(float(ref))
    for got, want in ((a.grad, dimg), (b.grad, dtxt), (s.grad.reshape(1), dls.reshape(1))):
        assert float((got.double() - want).abs().max()) < 1e-5 * float(want.abs().max())


def test_loss_class_takes_comm_and_reports_whether_it_needs_logits():
    _paths()
    from mmgclip.loss.loss_controller import create_loss
    cls = create_loss("AveragedMedicalCLIPLoss")

    class _Comm:
        def __init__(self, active):
            self.active, self.rank, self.world_size = active, 0, 2 if active else 1
    assert cls().needs_logits and cls(fused=False).needs_logits and cls(comm=None).needs_logits
    assert not cls(fused=True).needs_logits
    assert not cls(comm=_Comm(True)).needs_logits and cls(comm=_Comm(False)).needs_logits
    crit = cls(similarity_threshold=0.5, comm=_Comm(False), fused=True)
    assert crit.similarity_threshold == 0.5 and crit.fused is True


def test_bad_arguments_are_rejected_without_a_gpu():
    _paths()
    from mmgclip import _hip
    lib = _hip.load()
    assert lib.mmg_clip_labelled_rows_fwd(None, None, None, None, 8, 8, 100, None, None, None) != 0
    assert b"multiple of 32" in lib.mmg_last_error()
    assert lib.mmg_clip_labelled_rows_bwd_row(None, None, None, None, None, None, 1.0, 8, 0, 64, 0, None, None, None) != 0
    assert b"must be positive" in lib.mmg_last_error()
    assert lib.mmg_clip_labelled_rows_bwd_col(None, None, None, None, None, None, 0, None, 0, None, 1.0, 8, 8, 64, 0, None, None) != 0
    assert b"null pointer" in lib.mmg_last_error()
    assert lib.mmg_cluster_centroids(None, None, 20000, 64, 3, None, None) != 0


class _TinyClip(torch.nn.Module):
    def __init__(self, config=None):
        super().__init__()
        self.text_encoder = torch.nn.Linear(16, 8, bias=False)
        self.logit_scale = torch.nn.Parameter(torch.tensor(2.0))

    def count_parameters(self, model):
        return 0


class _LocalOnlyLoss(torch.nn.Module):
    """A criterion whose constructor cannot take `comm`."""

    def __init__(self):
        super().__init__()


class _FakeComm:
    rank, world_size, active, group = 0, 4, True, None


@pytest.mark.parametrize("loss_cls,global_loss,want", [(_LocalOnlyLoss, True, 0.25), (_LocalOnlyLoss, False, 0.25), (None, True, 1.0),
                                                        (None, False, 0.25)])
def test_grad_sync_averages_for_a_criterion_without_comm(tmp_path, monkeypatch, loss_cls, global_loss, want):
    """`ClassifierExperiment._grad_sync`: a criterion that could not take `comm` is a local-batch loss on every rank, so the gradients
    are averaged (scale 1/world) whatever `distributed.global_loss` says; one that takes it keeps sum / mean by that key."""
    _paths()
    from mmgclip.config import compose
    from mmgclip.experiments import ClassifierExperiment as CE
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(CE, "model", _TinyClip)
    if loss_cls is not None:
        monkeypatch.setattr(CE, "create_loss", lambda name: loss_cls)
    cfg = compose(os.path.join(ROOT, "mmg-clip_amd", "configs"), "train_binary_class_clf",
                  [f"checkpoints.checkpoints_export_dir={tmp_path}", f"base.tensorboard_export_dir={tmp_path}", "loss=averaged"]
                  + ([] if global_loss else ["distributed.global_loss=false"]))
    exp = CE.ClassifierExperiment(config=cfg, train_dataloader=[], comm=_FakeComm())
    if loss_cls is None:
        assert type(exp.criterion).__name__ == "AveragedMedicalCLIPLoss"
        assert (exp.criterion.comm is not None) == global_loss and exp.criterion.needs_logits == (not global_loss)
    assert exp._grad_sync().scale == want
