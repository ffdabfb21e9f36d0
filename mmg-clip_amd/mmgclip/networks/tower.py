"""What the encoder towers (convnext.py, vit.py, bert.py, resnet.py) share on the host side.

* `Tower`: the parameters bound into one flat arena (params.ParamArena), the cache of the working copies the kernels read, and the
  bookkeeping of a forward recorded for autograd.  A tower supplies `self.model` and `_build_working_copies()`.
* `checkpoint_plan` / `forward_parts` / `backward_parts`: a batch run in micro-batches ("parts"), with gradient checkpointing at that
  granularity.  Which part is recomputed, and in which order the backward takes them, is plain Python: tests/test_tower_cpu.py drives
  it with fakes.
* `conv_weight_rows` / `fold_conv_grad`: a stride = kernel (or im2col'd) convolution as a GEMM - its weight as GEMM rows, and the
  GEMM-shaped weight gradient folded back into torch's layout.
"""
import os

import torch
import torch.nn as nn

from .. import augment as AUG
from .. import kernels as K
from .._hip import call, ptr, stream
from ..params import ParamArena, note_forward, stream_anchor


class Tower(nn.Module):
    def __init__(self):
        super().__init__()
        self._arena = self._wc = self._wc_version = None
        self.post_backward_hook = None      # called with the arena once this tower's gradients are complete
        # pixel towers: seeded augmentation inside the stem's patchify (mmgclip/augment.py); acts in training mode only
        self.augment = None
        self.next_augment_seed = None       # tests: force the seed of the next forward that augments
        self._augment_seeds = AUG.AugmentSeeds()

    @property
    def arena(self):
        return self._arena

    def _arena_parameters(self):
        """Ordered (name, parameter) list that goes into the arena: what the tower trains, in the order its kernels want."""
        return list(self.model.named_parameters())

    def _materialize(self, device):
        """Bind the parameters into an arena on `device`; again whenever they were moved or replaced behind the arena's back."""
        if self._arena is not None and self._arena.device == device and self._arena.is_bound():
            return
        self._arena = ParamArena(self._arena_parameters(), device)
        self._wc_version = None
        self._bound()

    def _bound(self):
        """Called after every (re)build of the arena."""

    def _working_copy_key(self):
        """The working copies are current while this value stays the same."""
        return self._arena.version()

    def _refresh_working_copies(self):
        """bf16 / transposed / packed copies the kernels read (`self._wc`); rebuilt only when a parameter changed."""
        v = self._working_copy_key()
        if self._wc_version == v:
            return
        self._wc = self._build_working_copies()
        self._wc_version = v

    def set_augment(self, augment):
        """None | AugmentSpec | mapping (networks.image_encoder.augment) -> self.augment, validated."""
        self.augment = AUG.make_spec(augment)

    def augment_active(self):
        return self.training and self.augment is not None

    def _draw_augment(self, count, sample_ids):
        """One draw per forward: -> (geom rows, tone rows) of its `count` images, or None when no augmentation acts.  sample_ids: the number
        under which image i draws, default i - its position in this input."""
        if not self.augment_active():
            return None
        if self.next_augment_seed is not None:
            seed, self.next_augment_seed = int(self.next_augment_seed), None
        else:
            seed = self._augment_seeds.draw()
        ids = list(range(count)) if sample_ids is None else [int(i) for i in sample_ids]
        if len(ids) != count:
            raise ValueError(f"sample_ids names {len(ids)} images, the input holds {count}")
        return AUG.draw(self.augment, seed, ids)

    def _record_forward(self, device, wants_grad=True):
        """Start of a forward on `device` (the input's): -> the stream anchor the tower's autograd Function takes when this forward is
        recorded for a backward, else None."""
        self._materialize(device)
        needs_grad = torch.is_grad_enabled() and wants_grad and self._arena.any_trainable()
        note_forward(self, needs_grad)
        return stream_anchor(self, device) if needs_grad else None


# ---- pixels in ------------------------------------------------------------------------------------------------------------------------
def as_pixels(t):
    """fp32 in [0, 1], or raw uint16 / uint8, stay as they are (the stem's patchify reads all three); anything else becomes fp32."""
    return t if t.dtype in K.PIXEL_KINDS else t.float()


def augment_tables(rows, micro_batches, device):
    """rows: Tower._draw_augment's (geom, tone), one row per input image; micro_batches: per micro-batch the input indices of its images.
    -> per micro-batch (geom int32 [k, 4], tone fp32 [k, 2]) on `device`: the rows are put into processing order on the host and
    uploaded ONCE, every micro-batch gets a slice (a view) of that upload."""
    order = [i for idx in micro_batches for i in idx]
    geom = torch.tensor([rows[0][i] for i in order], dtype=torch.int32).reshape(-1, 4).to(device)
    tone = torch.tensor([rows[1][i] for i in order], dtype=torch.float32).reshape(-1, 2).to(device)
    out, start = [], 0
    for idx in micro_batches:
        out.append((geom[start:start + len(idx)], tone[start:start + len(idx)]))
        start += len(idx)
    return out


# ---- micro-batches and gradient checkpointing ---------------------------------------------------------------------------------------
# Checkpointing keeps only what rebuilds a part's input (its pixels) and re-runs the part's forward, activations saved, right before its
# backward: activation memory becomes one part's instead of the whole batch's.  The LAST part keeps its activations and the backward
# starts with it (reverse order), so still only one part's activations are alive at any time, and one of the n recomputations is not run.
def checkpoint_plan(n_parts, ckpt, keep_last):
    """-> (recompute: one flag per part, order: the parts as the backward takes them)."""
    if not ckpt:
        return [False] * n_parts, list(range(n_parts))
    recompute = [True] * n_parts
    if keep_last and n_parts:
        recompute[-1] = False
    return recompute, list(range(n_parts - 1, -1, -1))


class Recompute:
    """Record of a part that saved nothing: `part()` builds its input again; rows: its share of the features."""

    def __init__(self, part, rows):
        self.part, self.rows = part, rows


class Recorded:
    """What `forward_parts` leaves for `backward_parts`: per part its row count and its record (saved state, or a Recompute)."""

    def __init__(self, rows, records, order):
        self.rows, self.records, self.order = rows, records, order


def forward_parts(parts, run, ckpt):
    """parts: zero-argument callables, each building one micro-batch's input (a slice, or a stack of images) when it is needed;
    run(x, saving) -> (features [rows, ...], saved state); ckpt: checkpoint this forward (MMG_CKPT_KEEP_LAST=0: every part is recomputed,
    the last one too - read here, once per forward).  -> (features of all parts, Recorded)."""
    keep_last = ckpt and os.environ.get("MMG_CKPT_KEEP_LAST", "1") != "0"
    recompute, order = checkpoint_plan(len(parts), ckpt, keep_last)
    feats, records = [], []
    for part, again in zip(parts, recompute):
        x = part()
        feat, saved = run(x, not again)
        feats.append(feat)
        records.append(Recompute(part, feat.shape[0]) if again else saved)
        del x, saved
    return (torch.cat(feats, 0) if len(feats) > 1 else feats[0]), Recorded([f.shape[0] for f in feats], records, order)


def backward_parts(rec, dfeat, recompute_run, bwd):
    """dfeat: gradient of forward_parts' features; recompute_run(x) -> saved state; bwd(dfeat's rows of the part, saved state, last):
    last is True in the final call.  Every record is dropped as soon as its backward has returned."""
    starts = [sum(rec.rows[:k]) for k in range(len(rec.rows))]
    for pos, k in enumerate(rec.order):
        saved, rec.records[k] = rec.records[k], None
        if isinstance(saved, Recompute):
            saved = recompute_run(saved.part())
        bwd(dfeat[starts[k]:starts[k] + rec.rows[k]].contiguous(), saved, pos == len(rec.order) - 1)
        del saved


# ---- a convolution as a GEMM ----------------------------------------------------------------------------------------------------------
def conv_weight_rows(weight, cin_pad=None):
    """fp32 [Cout, Cin, kh, kw] -> [Cout, (kh, kw, ci)] contiguous (input channels zero-padded to cin_pad), K zero-padded to a multiple
    of 32 (the MFMA k-step)."""
    co, ci, kh, kw = weight.shape
    if cin_pad and cin_pad > ci:
        weight = torch.cat([weight, torch.zeros(co, cin_pad - ci, kh, kw, device=weight.device)], 1)
    w = weight.permute(0, 2, 3, 1).reshape(co, -1)
    k = w.shape[1]
    kp = (k + 31) // 32 * 32
    if kp == k:
        return w.contiguous()
    rows = torch.zeros(co, kp, device=w.device)
    rows[:, :k] = w
    return rows


def fold_conv_grad(tmp, grad, cout, cin, kh, kw):
    """Fold the GEMM-shaped weight gradient tmp [Cout, >= kh*kw*Cin] (columns (kh, kw, ci); a zero-padded tail is dropped) into the
    torch-layout gradient `grad` [Cout, Cin, kh, kw] (accumulating)."""
    kk = kh * kw * cin
    if tmp.shape[1] != kk:
        tmp = tmp[:, :kk].contiguous()
    call("mmg_grad_relayout", ptr(tmp), ptr(grad), 0, cout, cin, kh, kw, kk, stream())
