"""Loss classes with the reference's names, constructor and call signatures (mmgclip/loss/losses.py:6-216), computing
on the fp32 MI355X head kernels.  All return `(loss: 0-d tensor, labels: int64 [n])`.

`criterion(**outputs)` works exactly as in mmgclip/experiments/ClassifierExperiment.py:112.  When the model was run
with `materialize_logits=False` the CLIP loss and the averaged loss take their fused paths (no [n,n] logit matrices in HBM)."""
import torch
import torch.nn as nn

from .. import head


class CLIPLoss(nn.Module):
    """(CE(logits_per_image, arange) + CE(logits_per_text, arange)) / 2 — losses.py:28-44 (labels live on the logits'
    device instead of the reference's hard-coded `.cuda()`)."""

    def __init__(self, comm=None):
        super().__init__()
        self.comm = comm          # mmgclip.distributed.Comm for the global-batch loss (None = local batch)

    def forward(self, logits_per_image=None, logits_per_text=None, **kwargs):
        if logits_per_image is None or (self.comm is not None and self.comm.active):
            ie, te, s = kwargs["image_embeddings"], kwargs["text_embeddings"], kwargs["logit_scale"]
            loss = head.fused_clip_loss(ie, te, s, self.comm)
            n = ie.shape[0]
            off = 0 if self.comm is None else self.comm.rank * n
            return loss, torch.arange(off, off + n, device=ie.device)
        n, _ = logits_per_image.shape
        labels = torch.arange(n, device=logits_per_image.device)
        loss_i = head.cross_entropy(logits_per_image)
        loss_t = head.cross_entropy(logits_per_text)
        return (loss_i + loss_t) / 2, labels


class MMGCLIPLoss(nn.Module):
    """CLIP loss on recomputed logits + t2t_weight * symmetric CE between the two text views — losses.py:57-96."""

    def __init__(self, t2t_weight=0.5, comm=None):
        super().__init__()
        self.t2t_weight = t2t_weight
        self.comm = comm

    def forward(self, image_embeddings, text_embeddings, text_embeddings2, logit_scale, **kwargs):
        loss_clip = head.fused_clip_loss(image_embeddings, text_embeddings, logit_scale, self.comm)
        loss_t2t = head.fused_clip_loss(text_embeddings2, text_embeddings, logit_scale, self.comm)
        n = image_embeddings.shape[0]
        return loss_clip + loss_t2t * self.t2t_weight, torch.arange(n, device=image_embeddings.device)


class AveragedMedicalCLIPLoss(nn.Module):
    """Text-similarity label clustering + column-averaged logits — losses.py:98-216.

    Everything runs on the device: similarities (fp32 MFMA head kernel), the greedy threshold clustering
    (`mmg_greedy_threshold_labels`: the reference's Python double loop with one device read per element, losses.py:148-162,
    as one kernel; the only host traffic is the 4-byte cluster count), the per-cluster column means and both cross-entropies.
    `_assign_labels` / `_average_logits` keep the reference's signatures (a list of labels in and out) for callers that use
    the helpers directly.

    Two paths.  The dense one takes the model's materialised [n,n] logits (the reference's call).  The fused one
    (`head.fused_averaged_loss`) runs from the normalised embeddings, puts no [n,N] logit matrix in HBM and, with a communicator,
    is the loss of the GLOBAL batch: the clusters, the averaged columns and the text-side targets are those of all ranks' reports.
    It is taken when the logits are absent, when `comm` is active, or when `fused` is true; `needs_logits` tells the caller
    whether `forward` will read the logits at all.
    """

    def __init__(self, similarity_threshold=0.65, comm=None, fused=None):
        super().__init__()
        self.similarity_threshold = similarity_threshold
        self.comm = comm          # mmgclip.distributed.Comm for the global-batch loss (None = local batch)
        self.fused = fused        # None / False: fused only when the logits are absent or comm is active

    def _takes_fused_path(self, have_logits):
        return (not have_logits) or (self.comm is not None and self.comm.active) or bool(self.fused)

    @property
    def needs_logits(self):
        return not self._takes_fused_path(True)

    def _mesaure_embeddings_similarity(self, embeddings):
        e = head.L2Normalize.apply(embeddings.detach())
        one = torch.ones(1, device=e.device)
        _, _, sim = head.rows_forward(e.contiguous(), e.contiguous(), one, 0, True)
        return sim

    def _assign_labels(self, cosine_sim_matrix, threshold=0.65):
        labels, _, _ = head.greedy_threshold_labels(cosine_sim_matrix, threshold)
        return labels.tolist()

    def _average_logits(self, logits, list_labels):
        labels = torch.as_tensor(list_labels, device=logits.device, dtype=torch.int64)
        k = int(labels.max().item()) + 1
        counts = torch.bincount(labels, minlength=logits.shape[1]).to(torch.int32)
        return head.ClusterMeanCols.apply(logits, labels, counts, k)

    def forward(self, image_embeddings, text_embeddings, logit_scale, logits_per_image=None, logits_per_text=None, **kwargs):
        if self._takes_fused_path(logits_per_image is not None and logits_per_text is not None):
            return head.fused_averaged_loss(image_embeddings, text_embeddings, logit_scale, self.similarity_threshold, self.comm)
        sim = self._mesaure_embeddings_similarity(text_embeddings)
        labels, counts, k = head.greedy_threshold_labels(sim, self.similarity_threshold)
        averaged = head.ClusterMeanCols.apply(logits_per_image, labels, counts, k)
        loss_i = head.cross_entropy(averaged, labels)
        loss_t = head.cross_entropy(logits_per_text, labels)      # as the reference: [n,n] logits vs cluster ids
        return (loss_i + loss_t) / 2, labels


class SigmoidCLIPLoss(nn.Module):
    """Sigmoid pairwise loss (SigLIP, Zhai et al. 2023): (1/N) sum_ij softplus(-y_ij (s <I_i,T_j> + b)).  The reference has no such
    loss; it is an additive choice next to the three softmax losses above.

    Every (image, text) pair is scored on its own, so nothing is normalised across the batch, several positives per row are natural
    and the global-batch form needs ONE exchange (the embedding all-gather).  `positives`:
      "diagonal"  pair (i, i) alone is positive;
      "clusters"  every pair whose texts fall into one cluster of `AveragedMedicalCLIPLoss`'s greedy threshold clustering
                  (`similarity_threshold`) is positive: duplicates of a prompt are no longer each other's negatives.
    There is one path, `head.fused_sigmoid_loss`, from the normalised embeddings; the [n,n] logits are never read.  The model
    supplies `logit_bias` (a learnable 0-d parameter it creates for this loss)."""

    needs_logits = False

    def __init__(self, positives="diagonal", similarity_threshold=0.65, comm=None):
        super().__init__()
        if positives not in head.SIGMOID_POSITIVES:
            raise ValueError(f"positives must be one of {head.SIGMOID_POSITIVES}, got {positives!r}")
        self.positives = positives
        self.similarity_threshold = similarity_threshold
        self.comm = comm          # mmgclip.distributed.Comm for the global-batch loss (None = local batch)

    def forward(self, image_embeddings, text_embeddings, logit_scale, logit_bias, **kwargs):
        return head.fused_sigmoid_loss(image_embeddings, text_embeddings, logit_scale, logit_bias, self.positives,
                                       self.similarity_threshold, self.comm)
