"""Pooling the views of an exam inside the training graph.

The reference joins the per-view `[768]` vectors of a study offline, under a frozen encoder: `StudyFeatureExtractor`
(mmgclip/networks/image_features.py:225-245) takes `torch.stack(features).max(0)[0]`, `.mean(0)`, the stack itself or the
concatenation and writes one file per study.  Here the same step sits between the image tower and the projection head, with a
backward, so that an exam of several views is one training sample:

    feat [V, F] (one row per view, the views of a study adjacent)  ->  pool_views(feat, counts, method)  ->  [S, F]  (or [S, k F])

`avgpool` / `maxpool` run on the HIP kernels of csrc/view_pool.hip (one launch per direction, every output element written once:
bit-reproducible); `stack` / `concat` need the same number of views in every study and are a reshape that autograd handles itself.
The offsets that say which rows belong to which study are built on the host from the batch's view counts - the host knows them, the
loader made the batch - and copied to the device once per step; nothing is read back.
"""
import torch

from .. import kernels as K

MODES = {"avgpool": 0, "maxpool": 1}
_SPELLINGS = {"avg": "avgpool", "avgpool": "avgpool", "max": "maxpool", "maxpool": "maxpool", "stack": "stack", "concat": "concat"}


def normalize_method(name):
    """`concatenate_features_method` as the configs spell it (the reference's yaml: avgpool / maxpool; exam-reports.yaml here: avg)
    -> avgpool | maxpool | stack | concat."""
    try:
        return _SPELLINGS[str(name)]
    except KeyError:
        raise ValueError("Not implemented feature vector concatenation method") from None       # the reference's wording (:245)


def study_offsets(counts):
    """View counts per study -> host int32 [S + 1] with offsets[0] = 0 and offsets[S] = V: study s owns rows offsets[s] .. offsets[s+1]-1."""
    counts = [int(c) for c in counts]
    if not counts:
        raise ValueError("a batch of studies must hold at least one study")
    if min(counts) < 1:
        raise ValueError(f"every study needs at least one view, got the counts {counts}")
    offs = torch.zeros(len(counts) + 1, dtype=torch.int32)
    offs[1:] = torch.tensor(counts, dtype=torch.int32).cumsum(0)
    return offs


def offsets_to_device(offsets, device):
    """One asynchronous copy from page-locked memory: no host synchronisation."""
    return offsets.pin_memory().to(device, non_blocking=True)


class ViewPool(torch.autograd.Function):
    """apply(feat fp32 [V, C], offsets int32 [S + 1] on the device, S, mode) -> [S, C]; mode 0 = mean, 1 = max.  Saved for the backward:
    the offsets and (max) the int32 argmax - not the features."""

    @staticmethod
    def forward(ctx, feat, offsets, S, mode):
        feat = feat.contiguous()
        out, argmax = K.view_pool_fwd(feat, offsets, S, mode)
        ctx.save_for_backward(offsets, *([argmax] if argmax is not None else []))
        ctx.V, ctx.mode = feat.shape[0], mode
        return out

    @staticmethod
    def backward(ctx, dout):
        offsets, *rest = ctx.saved_tensors
        dfeat = K.view_pool_bwd(dout.float().contiguous(), offsets, rest[0] if rest else None, ctx.V, ctx.mode)
        return dfeat, None, None, None


def pool_views(feat, counts, method, offsets=None):
    """feat [V, C]: per-view features, the views of one study adjacent, studies in batch order; counts: views per study (host ints).
    avgpool / maxpool -> [S, C] through ViewPool (`offsets`: `study_offsets(counts)` already on the device, when the caller copied it
    ahead of time); stack / concat -> [S, k C] when every study has k views."""
    method = normalize_method(method)
    counts = [int(c) for c in counts]
    host = study_offsets(counts)
    S, V = len(counts), int(host[-1])
    if feat.dim() != 2 or feat.shape[0] != V:
        raise ValueError(f"{V} views in the studies ({counts}) but the features are {tuple(feat.shape)}")
    if method in ("stack", "concat"):
        if len(set(counts)) != 1:
            raise ValueError(f"`{method}` needs the same number of views in every study, got the counts {counts}; "
                             "use avgpool or maxpool for exams with a varying number of views")
        return feat.reshape(S, counts[0] * feat.shape[1])
    if offsets is None:
        offsets = offsets_to_device(host, feat.device)
    return ViewPool.apply(feat.float(), offsets, S, MODES[method])
