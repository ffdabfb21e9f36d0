"""The fused AveragedMedicalCLIPLoss (`head.fused_averaged_loss`, csrc/averaged_head.hip) on the MI355X against
`oracle.clip_oracle.averaged_medical_clip_loss` and its autograd in float64.

Inputs are built so that the clustering cannot flip between fp32 and float64 (`clustered_inputs`: text rows are
normalize(prototype + 0.05 noise)); every test asserts on the host, in float64, that no off-diagonal cosine lies within 1e-3 of the
threshold - a condition on the inputs, not a tolerance.  The embeddings are leaves BEFORE normalisation, so `L2Normalize` is in the
chain.  Tolerances are LOSS_RTOL / GRAD_RTOL / GRAD_ATOL of tests/test_head_gpu.py (fp32 on the f32 MFMA against the fp32 / fp64
reference, to rounding)."""
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.test_averaged_fused_cpu import THRESHOLD, assert_threshold_margin, clustered_inputs, oracle_unsharded
from tests.test_head_gpu import GRAD_ATOL, GRAD_RTOL, LOSS_RTOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "mmg-clip_amd", "configs")
LS = float(np.log(1 / 0.07))

# (N, D, clusters): (8,32) one partial tile; (37,64) a partial row tile and a partial column tile; (130,160) more than one
# 128-column round and D/32 not a multiple of 4; (256,512) the product shape.  k = 1, k = 3 (centroid matrix far below one tile),
# k about N/4, and (130,160,40): cluster ids >= 32, so the text-side target column crosses a tile boundary.
# (37,1024): the widest D, the only one that takes the NDT = 8 backward (D = 32, 64 take NDT = 1, 160 NDT = 2, 512 NDT = 4).
CASES = [(8, 32, 1), (8, 32, 3), (37, 64, 1), (37, 64, 3), (37, 64, 9), (72, 64, 7), (72, 64, 18), (130, 160, 3), (130, 160, 40),
         (256, 512, 1), (256, 512, 3), (256, 512, 64), (37, 1024, 9)]


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_garbage():
    """The experiments and models built below are reference cycles holding device memory: collect them when the module is done, so
    that tests which read `torch.cuda.memory_allocated()` later in the session do not see them go at a moment of the collector's choosing."""
    yield
    import gc
    _case.cache_clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _case(N, D, groups):
    """Inputs and the float64 oracle of one case, computed once and shared (read-only) by the tests that need it."""
    img, txt = clustered_inputs(N, D, groups, seed=1000 * N + groups)
    assert_threshold_margin(txt)
    ls = torch.tensor(LS)
    return (img, txt, ls) + oracle_unsharded(img, txt, ls)


def _run_fused(dev, img, txt, ls, comm=None):
    from mmgclip import head
    a, b, s = img.to(dev).requires_grad_(True), txt.to(dev).requires_grad_(True), ls.to(dev).requires_grad_(True)
    loss, labels = head.fused_averaged_loss(head.L2Normalize.apply(a), head.L2Normalize.apply(b), s.exp(), THRESHOLD, comm)
    loss.backward()
    return loss.detach().cpu(), labels.cpu(), a.grad.cpu(), b.grad.cpu(), s.grad.cpu()


def _run_dense(dev, img, txt, ls):
    """The dense path of the class on the same inputs (materialised logits, ClusterMeanCols, two dense cross-entropies)."""
    from mmgclip import head
    from mmgclip.loss.loss_controller import create_loss
    a, b, s = img.to(dev).requires_grad_(True), txt.to(dev).requires_grad_(True), ls.to(dev).requires_grad_(True)
    ie, te = head.L2Normalize.apply(a), head.L2Normalize.apply(b)
    li, lt = head.ScaledLogits.apply(ie, te, s.exp())
    loss, labels = create_loss("AveragedMedicalCLIPLoss")(THRESHOLD)(image_embeddings=ie, text_embeddings=te, logit_scale=s.exp(),
                                                                        logits_per_image=li, logits_per_text=lt)
    loss.backward()
    return loss.detach().cpu(), labels.cpu(), a.grad.cpu(), b.grad.cpu(), s.grad.cpu()


def _excess(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 is what np.testing.assert_allclose(rtol, atol) accepts."""
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    return float(((got - want).abs() / (atol + rtol * want.abs())).max())


@pytest.mark.parametrize("N,D,groups", CASES)
def test_fused_loss_and_gradients_match_the_float64_oracle(dev, N, D, groups):
    """Loss, labels, dI, dT and d loss / d logit_scale against the float64 oracle, at the constants of tests/test_head_gpu.py.
    The dense path's figures on the same inputs are printed beside the fused path's (the fused path averages embeddings where the
    reference averages logits: one reassociation of a sum of at most N fp32 terms on each side).  Measured on an MI355X, largest
    error as a fraction of its bar over the 12 cases: fused loss 0.08, dI 0.05, dT 0.14, dls 0.002; dense 0.21, 0.01, 0.06, 0.004."""
    img, txt, ls, ref, ref_labels, dimg, dtxt, dls = _case(N, D, groups)
    assert int(ref_labels.max()) + 1 == groups
    loss, labels, gi, gt, gs = _run_fused(dev, img, txt, ls)
    d_loss, d_labels, d_gi, d_gt, d_gs = _run_dense(dev, img, txt, ls)
    figs = {}
    for name, rtol, atol, got, dense, want in (("loss", LOSS_RTOL, 1e-7, loss, d_loss, ref), ("dI", GRAD_RTOL, GRAD_ATOL, gi, d_gi, dimg),
                                               ("dT", GRAD_RTOL, GRAD_ATOL, gt, d_gt, dtxt), ("dls", GRAD_RTOL, 1e-6, gs, d_gs, dls)):
        figs[name] = (_excess(got, want, rtol, atol), _excess(dense, want, rtol, atol))
    print(f"averaged fused vs fp64 N={N} D={D} k={groups}: error / bar (fused, dense) " +
          ", ".join(f"{k} {v[0]:.3f} {v[1]:.3f}" for k, v in figs.items()))
    assert labels.dtype == torch.int64 and labels.tolist() == ref_labels.tolist() == d_labels.tolist()
    for name, (fused, _) in figs.items():
        assert fused <= 1.0, (name, figs)


@pytest.mark.parametrize("N,D", [(8, 32), (37, 64), (72, 64), (256, 512), (37, 1024)])
def test_every_text_its_own_cluster_is_clip_loss(dev, N, D):
    """k = N: the centroids are the texts, the labels arange, and the loss is CLIPLoss - loss and all three gradients agree with
    `head.fused_clip_loss` on the same inputs."""
    from mmgclip import head
    img, txt = clustered_inputs(N, D, N, seed=7 * N + D)
    assert_threshold_margin(txt)
    ls = torch.tensor(LS)
    loss, labels, gi, gt, gs = _run_fused(dev, img, txt, ls)
    a, b, s = img.to(dev).requires_grad_(True), txt.to(dev).requires_grad_(True), ls.to(dev).requires_grad_(True)
    ref = head.fused_clip_loss(head.L2Normalize.apply(a), head.L2Normalize.apply(b), s.exp())
    ref.backward()
    assert labels.tolist() == list(range(N))
    assert abs(loss.item() - ref.item()) <= LOSS_RTOL * abs(ref.item()) + 1e-7, (loss.item(), ref.item())
    np.testing.assert_allclose(gi.numpy(), a.grad.cpu().numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(gt.numpy(), b.grad.cpu().numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(gs.numpy(), s.grad.cpu().numpy(), rtol=GRAD_RTOL, atol=1e-6)


@pytest.mark.parametrize("N,D", [(8, 32), (37, 64), (256, 512)])
def test_one_cluster_image_side_term_is_identically_zero(dev, N, D):
    """k = 1: every row's softmax has one column, so lse1 == pos1 bitwise."""
    from mmgclip import head
    _, txt, _ = _case(N, D, 1)[:3]
    be = head._HipAveragedBackend
    g = torch.Generator().manual_seed(N)
    ie = head.L2Normalize.apply(torch.randn(N, D, generator=g).to(dev))
    te = head.L2Normalize.apply(txt.to(dev))
    labels, counts, k = be.cluster(te, THRESHOLD)
    assert k == 1 and labels.tolist() == [0] * N and counts[0].item() == N
    cent = be.centroids(te, labels, k)
    # a sequential fp32 sum of N terms and one division: |error| <= N 2^-24 sum|x| / N + 2^-24 |mean| <= (N + 1) 2^-24 mean|x|
    bound = (N + 1) * 2.0 ** -24 * te.double().abs().mean(0, keepdim=True)
    assert bool(((cent.double() - te.double().mean(0, keepdim=True)).abs() <= bound).all())
    lse, pos = be.rows_forward(ie, cent, torch.tensor([14.2857], device=dev), labels)
    assert torch.equal(lse, pos)


def test_two_runs_give_the_same_bits(dev):
    """Centroids (fixed summation order, no float atomics), labels, loss and the embedding gradients are bit-reproducible; dscale ends
    in a float atomicAdd, as FusedClipLoss's does, and is exempt."""
    from mmgclip import head
    img, txt, ls = _case(130, 160, 40)[:3]
    be = head._HipAveragedBackend
    te = head.L2Normalize.apply(txt.to(dev))
    cents = []
    for _ in range(2):
        labels, _, k = be.cluster(te, THRESHOLD)
        cents.append(be.centroids(te, labels, k))
    assert torch.equal(cents[0], cents[1])
    r1, r2 = _run_fused(dev, img, txt, ls), _run_fused(dev, img, txt, ls)
    for x, y in zip(r1[:4], r2[:4]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("P", [2, 4])
def test_rank_simulated_global_averaged_loss(dev, P):
    """P simulated ranks on one GPU (N = 72, n_loc = 36 / 18): the backend per slice with gathered operands; concatenated dI / dT,
    summed dscale and the loss equal the unsharded float64 oracle (gradients w.r.t. the normalised embeddings)."""
    from mmgclip import head
    from oracle import clip_oracle as O
    N, D = 72, 64
    img, txt = clustered_inputs(N, D, 7, seed=1)
    assert_threshold_margin(txt)
    ie, te = head.L2Normalize.apply(img.to(dev)), head.L2Normalize.apply(txt.to(dev))
    scale = torch.tensor([14.2857], device=dev)
    a, b = ie.cpu().double().requires_grad_(True), te.cpu().double().requires_grad_(True)
    s = scale.cpu().double().reshape(()).requires_grad_(True)
    ref, ref_labels = O.averaged_medical_clip_loss(a, b, s, s * a @ b.t(), s * b @ a.t(), THRESHOLD)
    ref.backward()
    be = head._HipAveragedBackend
    labels, counts, k = be.cluster(te, THRESHOLD)                 # every rank: the same gathered bits, the same kernels
    assert labels.cpu().tolist() == ref_labels.tolist() and k == 7
    cent = be.centroids(te, labels, k)
    nl = N // P
    sls = [slice(r * nl, (r + 1) * nl) for r in range(P)]
    fw = [(be.rows_forward(ie[sl].contiguous(), cent, scale, labels[sl].contiguous()),
           be.rows_forward(te[sl].contiguous(), ie, scale, labels[sl].contiguous())) for sl in sls]
    lse_i, lse_t = torch.cat([f[0][0] for f in fw]), torch.cat([f[1][0] for f in fw])          # the "all-gather" of exchange 2
    coef = 1.0 / (2 * N)
    loss = sum(be.loss_sum(f[0][0], f[0][1], f[1][0], f[1][1], coef) for f in fw)              # the scalar all-reduce
    assert abs(loss.item() - ref.item()) <= LOSS_RTOL * abs(ref.item()) + 1e-7
    ds = torch.zeros(1, device=dev)
    d_ie, d_te = torch.empty_like(ie), torch.empty_like(te)
    for r, sl in enumerate(sls):
        x, y, c = ie[sl].contiguous(), te[sl].contiguous(), labels[sl].contiguous()
        dx = be.rows_backward_row(x, cent, scale, lse_i[sl].contiguous(), c, None, coef, None, ds)
        d_ie[sl] = be.rows_backward_col(x, te, scale, lse_t, labels, None, r * nl, None, None, coef, dx)
        dy = be.rows_backward_row(y, ie, scale, lse_t[sl].contiguous(), c, None, coef, None, ds)
        d_te[sl] = be.rows_backward_col(cent[c].contiguous(), ie, scale, lse_i, labels, c, 0, counts, None, coef, dy)
    np.testing.assert_allclose(d_ie.cpu().numpy(), a.grad.numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(d_te.cpu().numpy(), b.grad.numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(ds.item(), s.grad.item(), rtol=GRAD_RTOL, atol=1e-6)


# ---- class and model ------------------------------------------------------------------------------------------------------------
def _small_bert(monkeypatch):
    from mmgclip.networks import bert
    orig = bert.BertConfigLite.__init__

    def small(self, **kw):
        kw.setdefault("num_hidden_layers", 2)
        kw.setdefault("vocab_size", 3000)
        orig(self, **kw)
    monkeypatch.setattr(bert.BertConfigLite, "__init__", small)


def test_class_runs_without_logits_and_matches_its_dense_path(dev, monkeypatch):
    """`create_loss("AveragedMedicalCLIPLoss")()(**model(batch, materialize_logits=False))` runs; on the outputs of ONE forward the
    fused and the dense path give the same labels and the same loss.  Both are fp32 evaluations of one quantity, each within
    LOSS_RTOL |loss| + 1e-7 of its float64 value (the bar of the oracle test above), so they differ by at most twice that."""
    from mmgclip.config import compose
    from mmgclip.dataset.synthetic import synthetic_batch
    from mmgclip.loss.loss_controller import create_loss
    from mmgclip.networks.mmgclip_model import MMGCLIP
    _small_bert(monkeypatch)
    torch.manual_seed(0)
    model = MMGCLIP(compose(CFG_DIR, "train_binary_class_clf", ["networks.text_encoder.random_init=true",
                                                               "tokenizer=bert_clinical_seqlen=77", "loss=averaged"]))
    cls = create_loss("AveragedMedicalCLIPLoss")
    assert cls().needs_logits and not cls(fused=True).needs_logits
    out = model(synthetic_batch(32, S=77, vocab_size=3000, seed=3), materialize_logits=False)
    assert "logits_per_image" not in out
    loss, labels = cls()(**out)                                    # raised TypeError before the fused path existed
    loss.backward()
    assert torch.isfinite(loss) and labels.shape == (32,) and model.image_projection_layer.layer.weight.grad is not None
    full = model(synthetic_batch(32, S=77, vocab_size=3000, seed=3))
    dense, dense_labels = cls()(**full)
    fused, fused_labels = cls(fused=True)(**full)                  # the same tensors, logits present but not read
    assert fused_labels.tolist() == dense_labels.tolist()
    assert abs(fused.item() - dense.item()) <= 2 * (LOSS_RTOL * abs(dense.item()) + 1e-7), (fused.item(), dense.item())


def test_experiment_step_with_fused_averaged_loss_asks_for_no_logits(dev, tmp_path, monkeypatch):
    """One ClassifierExperiment epoch of one step with loss=averaged: `loss.config.fused=true` never calls `head.ScaledLogits.apply`,
    the shipped config (neither key) materialises the logits once per step as before."""
    from mmgclip import head
    from mmgclip.config import compose
    from mmgclip.dataset.synthetic import SyntheticLoader
    from mmgclip.experiments.experiments_controller import create_experiment
    _small_bert(monkeypatch)
    calls = []
    orig = head.ScaledLogits.apply
    monkeypatch.setattr(head.ScaledLogits, "apply", staticmethod(lambda *a: (calls.append(1), orig(*a))[1]))
    for over, want_calls, want_needs in ((["loss.config.fused=true", "loss.config.similarity_threshold=0.7"], 0, False), ([], 1, True)):
        cfg = compose(CFG_DIR, "train_binary_class_clf", ["networks.text_encoder.random_init=true", "tokenizer=bert_clinical_seqlen=77",
                                                          "loss=averaged", f"checkpoints.checkpoints_export_dir={tmp_path}/ckpt",
                                                          f"base.tensorboard_export_dir={tmp_path}/tb"] + over)
        torch.manual_seed(0)
        exp = create_experiment("classification")(config=cfg, train_dataloader=SyntheticLoader(1, 8, seed=5, S=77, vocab_size=3000),
                                                  valid_dataloader=None, test_dataloader=None, tokenizer=None)
        assert type(exp.criterion).__name__ == "AveragedMedicalCLIPLoss" and exp.criterion.needs_logits == want_needs
        assert exp.criterion.similarity_threshold == (0.7 if over else 0.65)
        del calls[:]
        loss = exp.train()
        assert np.isfinite(loss) and len(calls) == want_calls, (over, loss, len(calls))


# ---- one-rank RCCL group, every exchange kept, in a fresh child process -----------------------------------------------------------
def _rccl_worker(port, q):
    for p in (ROOT, os.path.join(ROOT, "mmg-clip_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    try:
        from mmgclip import distributed, head
        comm = distributed.init_from_env("nccl", single_rank=True)
        assert comm.active and comm.world_size == 1 and torch.distributed.get_backend() == "nccl"
        dev = torch.device("cuda:0")
        img, txt = clustered_inputs(72, 64, 7, seed=1)
        ls = torch.tensor(LS)
        comm.report()
        with_comm = _run_fused(dev, img, txt, ls, comm)
        rep_avg = comm.report()
        plain = _run_fused(dev, img, txt, ls, None)
        a, b = img.to(dev).requires_grad_(True), txt.to(dev).requires_grad_(True)
        head.fused_clip_loss(head.L2Normalize.apply(a), head.L2Normalize.apply(b), ls.to(dev).exp(), comm).backward()
        rep_clip = comm.report()
        torch.cuda.synchronize()
        q.put(("ok", [t.numpy() for t in with_comm], [t.numpy() for t in plain], rep_avg, rep_clip))
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    except Exception as e:           # report instead of hanging the parent on q.get
        import traceback
        q.put(("error", traceback.format_exc(), repr(e), None, None))


def test_rccl_one_rank_group_same_result_and_the_exchanges_of_clip_loss(dev):
    """backend "nccl" (= RCCL), one rank, `always_exchange`: the embedding / LSE all-gathers and the loss all-reduce go through RCCL
    and leave loss and gradients as `comm=None` gives them; `Comm.report()` shows the calls and bytes of CLIPLoss at that shape."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    p = ctx.Process(target=_rccl_worker, args=(port, q))
    p.start()
    status, with_comm, plain, rep_avg, rep_clip = q.get(timeout=300)
    p.join(timeout=120)
    assert status == "ok", with_comm
    assert p.exitcode == 0
    assert with_comm[0] == plain[0] and with_comm[1].tolist() == plain[1].tolist()           # loss (a one-rank sum) and labels
    np.testing.assert_array_equal(with_comm[2], plain[2])                                     # dI, dT: no atomics, the same bits
    np.testing.assert_array_equal(with_comm[3], plain[3])
    np.testing.assert_allclose(with_comm[4], plain[4], rtol=GRAD_RTOL, atol=1e-6)             # dscale: float atomicAdd order
    assert rep_avg == rep_clip and rep_avg["all_gather_calls"] == 4 and rep_avg["all_reduce_calls"] == 1, (rep_avg, rep_clip)
    assert rep_avg["all_gather_bytes"] == 2 * (72 * 64 * 4) + 2 * (72 * 4) and rep_avg["all_reduce_bytes"] == 4
