"""Host side of the contrastive heads: autograd wrappers over the fp32 gfx950 kernels of csrc/clip_head.hip (CLIP),
csrc/averaged_head.hip (AveragedMedicalCLIP) and csrc/sigmoid_head.hip (sigmoid pairwise), which share the tile skeleton of
csrc/clip_tile.h, and the backend of the retrieval ranks at validation (csrc/retrieval_head.hip, same skeleton; mmgclip/retrieval.py)
and of the nearest-neighbour search (csrc/topk_head.hip, same skeleton; mmgclip/search.py) and of the linear probe
(csrc/probe_head.hip, same skeleton; mmgclip/probe.py).

Reference arithmetic (path:line in the reference tree):
    mmgclip/networks/mmgclip_model.py:128-136  normalise, exp(logit_scale), two logit matmuls
    mmgclip/loss/losses.py:36-44               CLIPLoss
PyTorch is used for allocation / stream / autograd plumbing only; every FLOP below runs in the HIP library.
"""
import torch

from . import _hip
from ._hip import call, ptr, stream


def _f32c(t):
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _gather_rows(comm, t):
    """`t` of every rank, rank-major (`t` itself without an active communicator)."""
    return comm.all_gather_rows(t) if comm is not None and comm.active else t


def _global_batch(comm, img, txt, *scalars):
    """What every fused loss starts from: (img, txt, img_all, txt_all, off, N, *scalars) - the local embeddings in fp32, both
    matrices gathered over the ranks (exchange 1), the offset of the local rows in them, the global row count and each scalar
    parameter as a [1] fp32 tensor."""
    img, txt = _f32c(img), _f32c(txt)
    n_loc = img.shape[0]
    active = comm is not None and comm.active
    off, N = (comm.rank * n_loc, n_loc * comm.world_size) if active else (0, n_loc)
    return (img, txt, _gather_rows(comm, img), _gather_rows(comm, txt), off, N, *(_f32c(s.reshape(1)) for s in scalars))


def _global_loss(comm, loss):
    """The ranks' partial losses summed: the GLOBAL loss, identical on every rank."""
    return comm.all_reduce_sum(loss) if comm is not None and comm.active else loss


class L2Normalize(torch.autograd.Function):
    """y = x / ||x||_2 per row (no epsilon) — mmgclip_model.py:128-129."""

    @staticmethod
    def forward(ctx, x):
        _hip.require_gpu(x)
        x = _f32c(x)
        y = torch.empty_like(x)
        norm = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
        call("mmg_l2norm_fwd", ptr(x), ptr(y), ptr(norm), x.shape[0], x.shape[1], stream())
        ctx.save_for_backward(y, norm)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, norm = ctx.saved_tensors
        dy = _f32c(dy)
        dx = torch.empty_like(y)
        call("mmg_l2norm_bwd", ptr(y), ptr(norm), ptr(dy), ptr(dx), y.shape[0], y.shape[1], stream())
        return dx


def rows_forward(x_loc, y_all, scale, diag_off=0, want_logits=False):
    """lse, pos (and logits) of s * x_loc @ y_all.T — one launch, no autograd."""
    n_loc, D = x_loc.shape
    N = y_all.shape[0]
    lse = torch.empty(n_loc, device=x_loc.device, dtype=torch.float32)
    pos = torch.empty(n_loc, device=x_loc.device, dtype=torch.float32)
    logits = torch.empty(n_loc, N, device=x_loc.device, dtype=torch.float32) if want_logits else None
    call("mmg_clip_rows_fwd", ptr(x_loc), ptr(y_all), ptr(scale), n_loc, N, D, diag_off, ptr(lse), ptr(pos),
         ptr(logits), N if want_logits else 0, stream())
    return lse, pos, logits


class ScaledLogits(torch.autograd.Function):
    """logits_per_image, logits_per_text = s * I @ T.t(), s * T @ I.t()  (mmgclip_model.py:135-136).

    Materialises both matrices ([n,k] and [k,n]; k = n in training) because the reference API returns them; the backward takes arbitrary
    upstream gradients of both (mmg_clip_rows_bwd_dense).
    """

    @staticmethod
    def forward(ctx, img, txt, scale):
        _hip.require_gpu(img, txt, scale)
        img, txt = _f32c(img), _f32c(txt)
        scale = _f32c(scale.reshape(1))
        _, _, li = rows_forward(img, txt, scale, 0, True)
        _, _, lt = rows_forward(txt, img, scale, 0, True)
        ctx.save_for_backward(img, txt, scale)
        return li, lt

    @staticmethod
    def backward(ctx, dli, dlt):
        img, txt, scale = ctx.saved_tensors
        n, D = img.shape
        k = txt.shape[0]                  # k != n for zero-shot prompt scoring (PromptClassifier): Li [n,k], Lt [k,n]
        dli = _f32c(dli) if dli is not None else None
        dlt = _f32c(dlt) if dlt is not None else None
        dimg = torch.empty_like(img)
        dtxt = torch.empty_like(txt)
        dscale = torch.zeros(1, device=img.device, dtype=torch.float32)
        # d img = s (dLi + dLt^T) T ; d txt = s (dLt + dLi^T) I ; ds counted once (first call)
        call("mmg_clip_rows_bwd_dense", ptr(img), ptr(txt), ptr(scale), ptr(dli), k, ptr(dlt), n, n, k, D,
             ptr(dimg), ptr(dscale), stream())
        call("mmg_clip_rows_bwd_dense", ptr(txt), ptr(img), ptr(scale), ptr(dlt), n, ptr(dli), k, k, n, D,
             ptr(dtxt), None, stream())
        return dimg, dtxt, dscale.reshape(())


class CrossEntropyRows(torch.autograd.Function):
    """mean_r ( logsumexp(z_r) - z_r[label_r] ) * weight — F.cross_entropy of losses.py:40-41 on device."""

    @staticmethod
    def forward(ctx, logits, labels, weight):
        _hip.require_gpu(logits)
        logits = _f32c(logits)
        rows, C = logits.shape
        if labels is not None:
            labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
        lse = torch.empty(rows, device=logits.device, dtype=torch.float32)
        loss = torch.zeros(1, device=logits.device, dtype=torch.float32)
        w = float(weight) / rows
        call("mmg_ce_rows_fwd", ptr(logits), C, ptr(labels), rows, C, w, ptr(lse), ptr(loss), stream())
        ctx.save_for_backward(logits, lse, labels if labels is not None else torch.empty(0))
        ctx.has_labels = labels is not None
        ctx.w = w
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        logits, lse, labels = ctx.saved_tensors
        rows, C = logits.shape
        gout = _f32c(gout.reshape(1))
        d = torch.empty_like(logits)
        call("mmg_ce_rows_bwd", ptr(logits), C, ptr(labels) if ctx.has_labels else None, ptr(lse), ptr(gout),
             ctx.w, rows, C, ptr(d), C, stream())
        return d, None, None


def cross_entropy(logits, labels=None, weight=1.0):
    return CrossEntropyRows.apply(logits, labels, weight)


class _HipHeadBackend:
    """The product arithmetic of the fused loss: three entry points of libmmgclip_hip.so.

    No product signature selects anything else; tests/test_distributed_cpu.py replaces this module attribute in its own worker
    processes to exercise the collective choreography below on CPU/gloo."""

    @staticmethod
    def rows_forward(x_loc, y_all, scale, diag_off):
        _hip.require_gpu(x_loc, y_all, scale)
        lse, pos, _ = rows_forward(x_loc, y_all, scale, diag_off)
        return lse, pos

    @staticmethod
    def loss_sum(lse_i, pos_i, lse_t, pos_t, coef):
        loss = torch.zeros(1, device=lse_i.device, dtype=torch.float32)
        call("mmg_clip_loss_reduce", ptr(lse_i), ptr(pos_i), ptr(lse_t), ptr(pos_t), lse_i.shape[0], coef, ptr(loss), stream())
        return loss

    @staticmethod
    def rows_backward(x_loc, y_all, scale, lse_row, lse_col, gout, coef, diag_off, want_dscale):
        n_loc, D = x_loc.shape
        dx = torch.empty_like(x_loc)
        dscale = torch.zeros(1, device=x_loc.device, dtype=torch.float32) if want_dscale else None
        call("mmg_clip_rows_bwd_fused", ptr(x_loc), ptr(y_all), ptr(scale), ptr(lse_row), ptr(lse_col), ptr(gout), coef,
             n_loc, y_all.shape[0], D, diag_off, ptr(dx), ptr(dscale), stream())
        return dx, dscale


class FusedClipLoss(torch.autograd.Function):
    """CLIPLoss over (already L2-normalised) embeddings without materialising logits.

    loss = 1/(2N) [ sum_i (lse_i(A) - A_ii) + sum_j (lse_j(A^T) - A_jj) ],  A = s I T^T   (losses.py:36-44)

    With a communicator the columns are the all-gathered embeddings of every rank: exchange 1
    gathers the normalised embeddings, exchange 2 the two log-sum-exp vectors; gradients w.r.t. the local
    embeddings are then complete locally (no reduce-scatter).  `comm=None` is the reference's local-batch loss.
    The returned loss is the GLOBAL mean (identical on every rank); gradients are d(global loss)/d(local rows),
    so parameter gradients must be SUMMED across ranks (mmgclip/distributed.py does that).  d loss / d scale is the
    LOCAL rows' share; summed over ranks it is the full derivative.
    """

    @staticmethod
    def forward(ctx, img, txt, scale, comm):
        be = _HipHeadBackend
        img, txt, img_all, txt_all, off, N, scale = _global_batch(comm, img, txt, scale)
        lse_i, pos_i = be.rows_forward(img, txt_all, scale, off)
        lse_t, pos_t = be.rows_forward(txt, img_all, scale, off)
        loss = be.loss_sum(lse_i, pos_i, lse_t, pos_t, 1.0 / (2.0 * N))
        lse_i_all, lse_t_all = _gather_rows(comm, lse_i), _gather_rows(comm, lse_t)
        loss = _global_loss(comm, loss)
        ctx.save_for_backward(img, txt, scale, img_all, txt_all, lse_i, lse_t, lse_i_all, lse_t_all)
        ctx.off, ctx.N, ctx.be = off, N, be
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        img, txt, scale, img_all, txt_all, lse_i, lse_t, lse_i_all, lse_t_all = ctx.saved_tensors
        gout = _f32c(gout.reshape(1))
        coef = 1.0 / (2.0 * ctx.N)
        dimg, dscale = ctx.be.rows_backward(img, txt_all, scale, lse_i, lse_t_all, gout, coef, ctx.off, True)
        dtxt, _ = ctx.be.rows_backward(txt, img_all, scale, lse_t, lse_i_all, gout, coef, ctx.off, False)
        return dimg, dtxt, dscale.reshape(()), None


def fused_clip_loss(image_embeddings, text_embeddings, logit_scale, comm=None):
    """CLIPLoss on normalised embeddings; `logit_scale` is the already exponentiated scale (a tensor)."""
    return FusedClipLoss.apply(image_embeddings, text_embeddings, logit_scale, comm)


def greedy_threshold_labels(sim, threshold):
    """losses.py:148-162 on the device: (labels int64 [n], counts int32 [n], k) — one 4-byte read-back for k."""
    sim = _f32c(sim.detach())
    n = sim.shape[0]
    labels = torch.empty(n, device=sim.device, dtype=torch.int64)
    counts = torch.empty(n, device=sim.device, dtype=torch.int32)
    k = torch.empty(1, device=sim.device, dtype=torch.int32)
    call("mmg_greedy_threshold_labels", ptr(sim), sim.stride(0), n, float(threshold), ptr(labels), ptr(counts), ptr(k), stream())
    return labels, counts, int(k.item())


class _HipAveragedBackend:
    """The product arithmetic of the fused AveragedMedicalCLIPLoss: the entry points of csrc/averaged_head.hip plus the similarity
    and clustering kernels the dense path already uses.  As with `_HipHeadBackend`, no product signature selects anything else;
    tests/test_averaged_fused_cpu.py replaces this module attribute in its worker processes (gloo, CPU)."""

    @staticmethod
    def cluster(txt_all, threshold):
        """(labels int64 [N], counts int32 [N], k) of the gathered text: the similarity exactly as
        `AveragedMedicalCLIPLoss._mesaure_embeddings_similarity` forms it (a transient [N,N] fp32, no autograd), then
        losses.py:148-162 as one kernel."""
        _hip.require_gpu(txt_all)
        e = L2Normalize.apply(txt_all.detach()).contiguous()
        one = torch.ones(1, device=e.device)
        _, _, sim = rows_forward(e, e, one, 0, True)
        return greedy_threshold_labels(sim, threshold)

    @staticmethod
    def centroids(txt_all, labels, k):
        N, D = txt_all.shape
        out = torch.empty(k, D, device=txt_all.device, dtype=torch.float32)
        call("mmg_cluster_centroids", ptr(txt_all), ptr(labels), N, D, k, ptr(out), stream())
        return out

    @staticmethod
    def rows_forward(x_loc, y, scale, row_label):
        _hip.require_gpu(x_loc, y, scale, row_label)
        n_loc, D = x_loc.shape
        lse = torch.empty(n_loc, device=x_loc.device, dtype=torch.float32)
        pos = torch.empty(n_loc, device=x_loc.device, dtype=torch.float32)
        call("mmg_clip_labelled_rows_fwd", ptr(x_loc), ptr(y), ptr(scale), ptr(row_label), n_loc, y.shape[0], D, ptr(lse), ptr(pos),
             stream())
        return lse, pos

    loss_sum = staticmethod(_HipHeadBackend.loss_sum)

    @staticmethod
    def rows_backward_row(x_loc, y, scale, lse_row, row_label, gout, coef, dx, dscale):
        """ROW product; `dx` None = a fresh buffer, else accumulated into; `dscale` (a [1] tensor or None) is accumulated."""
        n_loc, D = x_loc.shape
        acc = dx is not None
        if dx is None:
            dx = torch.empty_like(x_loc)
        call("mmg_clip_labelled_rows_bwd_row", ptr(x_loc), ptr(y), ptr(scale), ptr(lse_row), ptr(row_label), ptr(gout), coef,
             n_loc, y.shape[0], D, int(acc), ptr(dx), ptr(dscale), stream())
        return dx

    @staticmethod
    def rows_backward_col(x_loc, y, scale, lse_col, col_label, row_key, key_off, counts, gout, coef, dx):
        """COL product; `row_key` None = key_off + r; `counts` None = weight 1, else 1 / counts[key]."""
        n_loc, D = x_loc.shape
        acc = dx is not None
        if dx is None:
            dx = torch.empty_like(x_loc)
        call("mmg_clip_labelled_rows_bwd_col", ptr(x_loc), ptr(y), ptr(scale), ptr(lse_col), ptr(col_label), ptr(row_key), key_off,
             ptr(counts), 0 if counts is None else counts.shape[0], ptr(gout), coef, n_loc, y.shape[0], D, int(acc), ptr(dx), stream())
        return dx


class FusedAveragedLoss(torch.autograd.Function):
    """AveragedMedicalCLIPLoss over (already L2-normalised) embeddings of the GLOBAL batch, no [n,N] logits (losses.py:164-216).

    loss = 1/(2N) [ sum_i (lse1_i - s <I_i, Tbar_c(i)>) + sum_j (lse2_j - s <T_j, I_c(j)>) ]
    c = greedy threshold labels of the gathered text, Tbar = cluster means of the text embeddings (the reference's column average
    of s I T^T, by linearity), lse1 / lse2 the row log-sum-exps of s I Tbar^T and s T I^T.  The exchanges are FusedClipLoss's:
    all-gather of the embeddings, all-gather of the two log-sum-exp vectors, all-reduce of the loss; every rank clusters the same
    gathered bits with the same deterministic kernels, so no collective's shape depends on k.  Gradients are for the local rows
    and complete locally; d loss / d scale is the local rows' share.  The labels carry no gradient.
    Returns (loss, global cluster ids of the local rows)."""

    @staticmethod
    def forward(ctx, img, txt, scale, threshold, comm):
        be = _HipAveragedBackend
        img, txt, img_all, txt_all, off, N, scale = _global_batch(comm, img, txt, scale)
        labels, counts, k = be.cluster(txt_all, threshold)
        cent = be.centroids(txt_all, labels, k)
        c_loc = labels[off:off + img.shape[0]].contiguous()
        lse_i, pos_i = be.rows_forward(img, cent, scale, c_loc)
        lse_t, pos_t = be.rows_forward(txt, img_all, scale, c_loc)
        loss = be.loss_sum(lse_i, pos_i, lse_t, pos_t, 1.0 / (2.0 * N))
        lse_i_all, lse_t_all = _gather_rows(comm, lse_i), _gather_rows(comm, lse_t)
        loss = _global_loss(comm, loss)
        ctx.save_for_backward(img, txt, scale, img_all, txt_all, cent, labels, counts, c_loc, lse_i, lse_t, lse_i_all, lse_t_all)
        ctx.off, ctx.N, ctx.be = off, N, be
        ctx.mark_non_differentiable(c_loc)
        return loss.reshape(()), c_loc

    @staticmethod
    def backward(ctx, gout, _dlabels):
        img, txt, scale, img_all, txt_all, cent, labels, counts, c_loc, lse_i, lse_t, lse_i_all, lse_t_all = ctx.saved_tensors
        be, off = ctx.be, ctx.off
        gout = _f32c(gout.reshape(1))
        coef = 1.0 / (2.0 * ctx.N)
        dscale = torch.zeros(1, device=img.device, dtype=torch.float32)
        dimg = be.rows_backward_row(img, cent, scale, lse_i, c_loc, gout, coef, None, dscale)
        dimg = be.rows_backward_col(img, txt_all, scale, lse_t_all, labels, None, off, None, gout, coef, dimg)
        dtxt = be.rows_backward_row(txt, img_all, scale, lse_t, c_loc, gout, coef, None, dscale)
        dtxt = be.rows_backward_col(cent[c_loc].contiguous(), img_all, scale, lse_i_all, labels, c_loc, 0, counts, gout, coef, dtxt)
        return dimg, dtxt, dscale.reshape(()), None, None


def fused_averaged_loss(image_embeddings, text_embeddings, logit_scale, threshold, comm=None):
    """AveragedMedicalCLIPLoss on normalised embeddings -> (loss, labels_of_local_rows); `logit_scale` is the exponentiated scale."""
    return FusedAveragedLoss.apply(image_embeddings, text_embeddings, logit_scale, float(threshold), comm)


class _HipSigmoidBackend:
    """The product arithmetic of the fused sigmoid pairwise loss: the two entry points of csrc/sigmoid_head.hip and the row reduction
    of the head.  As with `_HipHeadBackend`, no product signature selects anything else; tests/test_sigmoid_loss_cpu.py replaces this
    module attribute in its worker processes (gloo, CPU).  `row_key` / `col_label` None = the diagonal at `diag_off`."""

    @staticmethod
    def rows_forward(x_loc, y_all, scale, bias, row_key, col_label, diag_off):
        _hip.require_gpu(x_loc, y_all, scale, bias, row_key, col_label)
        n_loc, D = x_loc.shape
        row_loss = torch.empty(n_loc, device=x_loc.device, dtype=torch.float32)
        call("mmg_sigmoid_rows_fwd", ptr(x_loc), ptr(y_all), ptr(scale), ptr(bias), ptr(row_key), ptr(col_label), n_loc,
             y_all.shape[0], D, diag_off, ptr(row_loss), stream())
        return row_loss

    @staticmethod
    def loss_sum(row_loss, coef):
        """coef * sum(row_loss): the head's one-workgroup reduction with a zero `pos`."""
        loss = torch.zeros(1, device=row_loss.device, dtype=torch.float32)
        call("mmg_clip_loss_reduce", ptr(row_loss), ptr(torch.zeros_like(row_loss)), None, None, row_loss.shape[0], coef, ptr(loss),
             stream())
        return loss

    @staticmethod
    def rows_backward(x_loc, y_all, scale, bias, row_key, col_label, gout, coef, diag_off, dscale=None, dbias=None):
        """dX (fresh); `dscale` / `dbias` ([1] tensors or None) are accumulated into."""
        n_loc, D = x_loc.shape
        dx = torch.empty_like(x_loc)
        call("mmg_sigmoid_rows_bwd", ptr(x_loc), ptr(y_all), ptr(scale), ptr(bias), ptr(row_key), ptr(col_label), ptr(gout), coef,
             n_loc, y_all.shape[0], D, diag_off, ptr(dx), ptr(dscale), ptr(dbias), stream())
        return dx


SIGMOID_POSITIVES = ("diagonal", "clusters")


class FusedSigmoidLoss(torch.autograd.Function):
    """Sigmoid pairwise loss (SigLIP, Zhai et al. 2023) over (already L2-normalised) embeddings of the GLOBAL batch, no [n,N] matrix.

    loss = (1/N) sum_{i,j} softplus(-y_ij (s <I_i, T_j> + b)),  y_ij = +1 for a positive pair, -1 otherwise, N = global rows.
    positives "diagonal": pair (i, i).  "clusters": every (i, j) whose texts fall into one greedy-threshold cluster, the clustering
    of `FusedAveragedLoss` (same kernels, same threshold) on the gathered text - every rank clusters the same bits.
    ONE exchange: the all-gather of the two embedding matrices (plus the all-reduce of the scalar loss); a pair's term needs no
    normaliser from another rank.  Gradients are d(global loss)/d(local rows) and complete locally; d loss / d scale and d loss / d bias
    are the LOCAL rows' share (counted once, by the image-side launch) and are summed over ranks by GradSync.  The labels carry no
    gradient.  Returns (loss, labels of the local rows)."""

    @staticmethod
    def forward(ctx, img, txt, scale, bias, positives, threshold, comm):
        be, cl = _HipSigmoidBackend, _HipAveragedBackend
        if positives not in SIGMOID_POSITIVES:
            raise ValueError(f"positives must be one of {SIGMOID_POSITIVES}, got {positives!r}")
        img, txt, img_all, txt_all, off, N, scale, bias = _global_batch(comm, img, txt, scale, bias)
        n_loc = img.shape[0]
        if positives == "clusters":
            labels, _, _ = cl.cluster(txt_all, threshold)
            labels = labels.contiguous()
            key = labels[off:off + n_loc].contiguous()
            out_labels = key
        else:
            labels = key = None
            out_labels = torch.arange(off, off + n_loc, device=img.device)
        row_loss = be.rows_forward(img, txt_all, scale, bias, key, labels, off)
        loss = _global_loss(comm, be.loss_sum(row_loss, 1.0 / N))
        saved = [img, txt, scale, bias, img_all, txt_all] + ([key, labels] if labels is not None else [])
        ctx.save_for_backward(*saved)
        ctx.off, ctx.N, ctx.be = off, N, be
        ctx.mark_non_differentiable(out_labels)
        return loss.reshape(()), out_labels

    @staticmethod
    def backward(ctx, gout, _dlabels):
        img, txt, scale, bias, img_all, txt_all = ctx.saved_tensors[:6]
        key, labels = ctx.saved_tensors[6:] if len(ctx.saved_tensors) > 6 else (None, None)
        be, off = ctx.be, ctx.off
        gout = _f32c(gout.reshape(1))
        coef = 1.0 / ctx.N
        dscale = torch.zeros(1, device=img.device, dtype=torch.float32)
        dbias = torch.zeros(1, device=img.device, dtype=torch.float32)
        # y is symmetric (j == off + i  <=>  i == j - off; label equality), so the same keys serve both sides; every pair's share of
        # the two scalars is counted once, by the image-side launch
        dimg = be.rows_backward(img, txt_all, scale, bias, key, labels, gout, coef, off, dscale, dbias)
        dtxt = be.rows_backward(txt, img_all, scale, bias, key, labels, gout, coef, off, None, None)
        return dimg, dtxt, dscale.reshape(()), dbias.reshape(()), None, None, None


def fused_sigmoid_loss(image_embeddings, text_embeddings, logit_scale, logit_bias, positives="diagonal", threshold=0.65, comm=None):
    """Sigmoid pairwise loss on normalised embeddings -> (loss, labels_of_local_rows); `logit_scale` is the exponentiated scale."""
    return FusedSigmoidLoss.apply(image_embeddings, text_embeddings, logit_scale, logit_bias, positives, float(threshold), comm)


class _HipRetrievalBackend:
    """The product arithmetic of the retrieval metrics (mmgclip/retrieval.py): the one entry point of csrc/retrieval_head.hip.  As with
    `_HipHeadBackend`, no product signature selects anything else; tests/test_retrieval_cpu.py replaces this module attribute in its
    worker processes (gloo, CPU).  `row_key` / `col_label` None = the diagonal at `diag_off`."""

    @staticmethod
    def rank(x_loc, y_all, row_key, col_label, diag_off):
        """(best fp32, n_pos, n_gt, n_eq int32), each [n_loc]: the best positive score of every local query and the negatives of
        the gallery above / at it.  No autograd, no [n_loc,N] allocation."""
        _hip.require_gpu(x_loc, y_all, row_key, col_label)
        n_loc, D = x_loc.shape
        best = torch.empty(n_loc, device=x_loc.device, dtype=torch.float32)
        n_pos, n_gt, n_eq = (torch.empty(n_loc, device=x_loc.device, dtype=torch.int32) for _ in range(3))
        call("mmg_retrieval_rows_rank", ptr(x_loc), ptr(y_all), ptr(row_key), ptr(col_label), n_loc, y_all.shape[0], D, diag_off,
             ptr(best), ptr(n_pos), ptr(n_gt), ptr(n_eq), stream())
        return best, n_pos, n_gt, n_eq


class _HipTopKBackend:
    """The product arithmetic of the nearest-neighbour search (mmgclip/search.py): the entry points of csrc/topk_head.hip.  As with
    `_HipRetrievalBackend`, no product signature selects anything else; tests/test_topk_cpu.py replaces this module attribute in its
    worker processes (gloo, CPU)."""

    @staticmethod
    def supported(D, k):
        """Whether one launch can hold the staged rows and the candidate lists for this (D, k).  No GPU is needed."""
        return bool(_hip.load().mmg_topk_rows_supported(int(D), int(k)))

    @staticmethod
    def topk(x_loc, y, k, exclude=0, row_key=None, col_label=None, diag_off=0, j_base=0, out=None):
        """(scores fp32 [n,k], indices int32 [n,k]): the k best columns of `y` for every row of `x_loc` under (score descending, global
        index j_base + j ascending), padded with -inf / -1.  exclude: 0 none, 1 the column diag_off + i, 2 col_label[j] == row_key[i].
        `out` = (scores, indices) of earlier calls over OTHER columns: merged in place and returned.  No autograd, no [n,N] allocation."""
        _hip.require_gpu(x_loc, y, row_key, col_label)
        n_loc, D = x_loc.shape
        if out is None:
            scores = torch.empty((n_loc, k), device=x_loc.device, dtype=torch.float32)
            indices = torch.empty((n_loc, k), device=x_loc.device, dtype=torch.int32)
        else:
            scores, indices = out
            _hip.require_gpu(scores, indices)
            if (scores.shape != (n_loc, k) or indices.shape != (n_loc, k) or scores.dtype != torch.float32 or indices.dtype != torch.int32
                    or not (scores.is_contiguous() and indices.is_contiguous())):
                raise ValueError("out must be contiguous (fp32 [n,k], int32 [n,k]) lists of earlier calls")
        call("mmg_topk_rows", ptr(x_loc), ptr(y), n_loc, y.shape[0], D, k, exclude, ptr(row_key), ptr(col_label), diag_off, j_base,
             0 if out is None else 1, ptr(scores), ptr(indices), stream())
        return scores, indices


class _HipProbeBackend:
    """The product arithmetic of the linear probe (mmgclip/probe.py): the entry points of csrc/probe_head.hip.  As with
    `_HipTopKBackend`, no product signature selects anything else; tests/test_probe_cpu.py replaces this module attribute in its
    worker processes (gloo, CPU)."""

    @staticmethod
    def supported(D, C):
        """Whether the fused kernel takes this (D, C): D a multiple of 32 in [32,1024], 2 <= C <= 32.  No GPU is needed."""
        return bool(_hip.load().mmg_probe_rows_supported(int(D), int(C)))

    @staticmethod
    def evaluate(x, W, b, labels, class_weight=None, n_groups=0):
        """fp64 [C (D+1) + 1] on the device: the un-normalised dW | db as [C, D+1] (column D is db), then the loss L, of the rows
        `x` [n,D] with int64 `labels` (-1 = ignored) at the fp32 weights W [C,D], b [C]; `class_weight` fp32 [C] or None.  One read
        of `x`, no [n,C] temporary, no atomics: the same bits from run to run.  n_groups: the persistent grid, 0 = one per CU."""
        _hip.require_gpu(x, W, b, labels, class_weight)
        n, D = x.shape
        C = W.shape[0]
        nbytes = _hip.load().mmg_probe_rows_partials_bytes(n, D, C, int(n_groups))
        if nbytes <= 0:
            raise ValueError(f"the probe kernel takes D % 32 == 0 in [32,1024], 2 <= C <= 32, n >= 1 and 0 <= n_groups <= 4096; "
                             f"got n={n} D={D} C={C} n_groups={n_groups}")
        partials = torch.empty(nbytes // 8, device=x.device, dtype=torch.float64)
        out = torch.empty(C * (D + 1) + 1, device=x.device, dtype=torch.float64)
        call("mmg_probe_rows", ptr(x), ptr(W), ptr(b), ptr(labels), ptr(class_weight), n, D, C, int(n_groups), ptr(partials), ptr(out),
             stream())
        return out


class _HipAurocBackend:
    """The product arithmetic of the zero-shot AUROC with bootstrap replicates (mmgclip/zeroshot_auroc.py): the two entry points of
    csrc/auroc_head.hip.  As with `_HipRetrievalBackend`, no product signature selects anything else; tests/test_auroc_cpu.py replaces
    this module attribute.  Weights are int8 [B, ld], replicate-major, ld a multiple of 16 with zeros in the padding."""

    @staticmethod
    def bootstrap_weights(seed, n, b0, B, device=None):
        """int8 [B, ceil16(n)]: how many of replicate b's n draws landed on sample t, b = b0 .. b0+B-1; padding columns 0.  A count
        above 127 comes back as -128: the caller raises on any negative weight (one read-back for all its chunks)."""
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        w = torch.empty((B, (n + 15) // 16 * 16), device=device, dtype=torch.int8)
        _hip.require_gpu(w)
        call("mmg_bootstrap_weights", int(seed) & 0xFFFFFFFFFFFFFFFF, n, b0, B, ptr(w), w.shape[1], stream())
        return w

    @staticmethod
    def pairs(s_pos, s_neg, w_pos, w_neg, neg_total=None):
        """int64 [B]: U2_b = sum_ij w_pos[b,i] w_neg[b,j] (2 [s+_i > s-_j] + [s+_i == s-_j]), exact.  The int32 accumulator bound
        2 max_b sum_j w_neg[b,j] < 2^31 is checked here: against `neg_total`, an upper bound of every replicate's negative weights
        that the caller can prove (a bootstrap of N draws: N), or, without one, by a device reduction read back (torch widens the
        int8 weights for it: a transient of 8 bytes per weight)."""
        _hip.require_gpu(s_pos, s_neg, w_pos, w_neg)
        s_pos, s_neg = _f32c(s_pos), _f32c(s_neg)
        P, Nn, B = s_pos.shape[0], s_neg.shape[0], w_neg.shape[0]
        if w_pos.dtype != torch.int8 or w_neg.dtype != torch.int8 or w_pos.shape[0] != B or not (w_pos.is_contiguous() and w_neg.is_contiguous()):
            raise ValueError("weights must be contiguous int8 [B, ld] with one row per replicate in both matrices")
        heaviest = int(w_neg.sum(dim=1, dtype=torch.int64).max()) if neg_total is None else int(neg_total)
        if 2 * heaviest >= 2 ** 31:
            raise ValueError(f"a replicate's negative weights sum to {heaviest}: 2 * that must stay below 2^31 (int32 accumulators)")
        partial = torch.empty(((P + 31) // 32, B), device=s_pos.device, dtype=torch.int64)
        call("mmg_auroc_pairs", ptr(s_pos), ptr(s_neg), ptr(w_pos), w_pos.shape[1], ptr(w_neg), w_neg.shape[1], P, Nn, B, ptr(partial),
             stream())
        return partial.sum(dim=0)


class ClusterMeanCols(torch.autograd.Function):
    """[n,N] logits -> [n,k] per-cluster column means (losses.py:164-186) and the matching gradient."""

    @staticmethod
    def forward(ctx, logits, labels, counts, k):
        _hip.require_gpu(logits, labels, counts)
        logits = _f32c(logits)
        n, N = logits.shape
        out = torch.empty(n, k, device=logits.device, dtype=torch.float32)
        call("mmg_cluster_mean_cols_fwd", ptr(logits), logits.stride(0), n, N, ptr(labels), ptr(counts), k, ptr(out), k, stream())
        ctx.save_for_backward(labels, counts)
        ctx.shape = (n, N)
        return out

    @staticmethod
    def backward(ctx, dout):
        labels, counts = ctx.saved_tensors
        n, N = ctx.shape
        dout = _f32c(dout)
        dl = torch.empty(n, N, device=dout.device, dtype=torch.float32)
        call("mmg_cluster_mean_cols_bwd", ptr(dout), dout.stride(0), n, N, ptr(labels), ptr(counts), ptr(dl), N, stream())
        return dl, None, None, None
