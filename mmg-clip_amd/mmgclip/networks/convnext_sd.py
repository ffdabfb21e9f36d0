"""Stochastic depth of the ConvNeXt tower (torchvision `StochasticDepth(p, "row")` at the end of every CNBlock) - decided here, on the
host, as plain values (no tensors, no device), in the style of convnext_plan.py.

  * `block_rates`   p_b = rate * b / (B - 1) over the tower's B blocks (torchvision's linear rule; p_0 = 0, p_{B-1} = rate);
  * `keep_matrix`   which sample survives which block: the counter-based hash of csrc/dropout.h (restated in its few integer lines; the
                    test oracle oracle/dropout_oracle.py restates it too), keyed by (seed, site = block number) and indexed by the
                    sample's position in the forward's INPUT - so a mask does not depend on the micro-batch size, on the grouping of a
                    list of images by size, or on whether a pass is a checkpointed recomputation;
  * `schedule`      per micro-batch: the tower never computes a dropped sample.  Its kernels treat images independently, so before a
                    block the images are swapped in place until the kept ones are a contiguous prefix, the block runs on that prefix,
                    and the tail is copied through.  The images stay where the swaps left them (the next block swaps from there); the
                    features leave in that order and `processing_order` routes them back.  ConvNextTower._forward_mb / _backward_mb
                    only execute this record;
  * `DropSeeds`     one seed per recorded forward from a generator the tower owns, derived from (base seed, rank) the way
                    BertTower.reseed_dropout derives its own (a different stream: the two towers' draws are unrelated).
A kept sample gets x + (gamma / (1 - p_b)) * branch(x): the factor is the same for every kept sample of a block, so it is folded into the
layer scale the kernels read (`scales`)."""
import os
from typing import NamedTuple, Tuple

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def check_rate(rate):
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"stochastic_depth_prob must be in [0, 1), got {rate}")
    return rate


def block_rates(rate, depths):
    """p_b for b = 0 .. B-1, B = sum(depths)."""
    B = sum(depths)
    return [rate * b / (B - 1.0) for b in range(B)] if B > 1 else [rate] * B


def scales(rate, depths):
    """1 / (1 - p_b): what a kept sample's branch is multiplied by."""
    return [1.0 / (1.0 - p) for p in block_rates(rate, depths)]


# ---- the mask: csrc/dropout.h in numpy ----------------------------------------------------------------------------------------------
def _fmix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    return x ^ (x >> np.uint64(16))


def drop_key(seed, site):
    """mmg_drop_key(seed, site)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return int(_fmix32(((int(site) ^ (seed >> 32)) + (seed & 0xFFFFFFFF)) & 0xFFFFFFFF))


def drop_threshold(p):
    """mmg_drop_threshold(p): p is a C float there."""
    t = float(np.float32(p)) * 4294967296.0
    return 0 if t <= 0.0 else (4294967295 if t >= 4294967295.0 else int(t))


def keep_matrix(seed, sample_ids, rates):
    """bool [B, n]: keep[b, i] = mmg_drop_bits(sample_ids[i], mmg_drop_key(seed, b)) >= mmg_drop_threshold(rates[b])."""
    ids = np.asarray(sample_ids, dtype=np.uint64).reshape(-1) & _M32
    keep = np.empty((len(rates), ids.size), dtype=bool)
    for b, p in enumerate(rates):
        bits = _fmix32((ids * np.uint64(0x9E3779B1) + np.uint64(drop_key(seed, b))) & _M32)
        keep[b] = bits >= np.uint64(drop_threshold(p))
    return keep


# ---- the schedule of one micro-batch ------------------------------------------------------------------------------------------------
class BlockStep(NamedTuple):
    n_k: int                            # samples the block keeps: after the swaps they are images 0 .. n_k-1
    pairs: Tuple[Tuple[int, int], ...]  # disjoint (i, j), i < n_k <= j: image i (dropped) and image j (kept) change places before the block
    offset: int                         # where these pairs start in Schedule.table, counted in pairs


class Schedule(NamedTuple):
    n: int
    steps: Tuple[BlockStep, ...]        # one per block, in forward order
    table: Tuple[int, ...]              # every block's pairs, flattened (i0, j0, i1, j1, ...): ONE int32 upload per micro-batch
    perm: Tuple[int, ...]               # perm[slot] = position (in the micro-batch's input) of the image that ends in `slot`


def schedule(keep):
    """keep: bool [B, n] of ONE micro-batch (column i = its i-th input image) -> Schedule.  Per block at most min(n_d, n_k) swaps: every
    dropped image inside the first n_k slots is exchanged with a kept image of the tail; nothing else moves."""
    keep = np.asarray(keep, dtype=bool)
    B, n = keep.shape
    order = list(range(n))              # order[slot] = input position of the image now in that slot
    steps, table = [], []
    for b in range(B):
        kept = [bool(keep[b, order[s]]) for s in range(n)]
        n_k = sum(kept)
        holes = [s for s in range(n_k) if not kept[s]]
        fills = [s for s in range(n_k, n) if kept[s]]
        pairs = tuple(zip(holes, fills))                # (equally many: the prefix lacks exactly the kept images that sit in the tail)
        steps.append(BlockStep(n_k, pairs, len(table) // 2))
        for i, j in pairs:
            order[i], order[j] = order[j], order[i]
            table += [i, j]
    return Schedule(n, tuple(steps), tuple(table), tuple(order))


def processing_order(micro_batches, schedules):
    """micro_batches: per micro-batch the input indices of its images, in the order it is given them; schedules: its Schedule.
    -> (order, inverse): order[pos] = input index of feature row `pos` as the micro-batches emit them, inverse[i] = the row of input i,
    so `features[inverse]` is in input order (the composition of the size grouping's permutation with every micro-batch's)."""
    order = [idx[s] for idx, sch in zip(micro_batches, schedules) for s in sch.perm]
    inverse = [0] * len(order)
    for pos, i in enumerate(order):
        inverse[i] = pos
    return order, inverse


# ---- seeds --------------------------------------------------------------------------------------------------------------------------
class DropSeeds:
    """The tower's private seed stream: restarted from (seed, rank) whenever `utils.global_utils.seeding` has run since the last draw, so
    `seeding(config.base.seed)` reproduces a run, torch's global generators are never consumed, and every data-parallel rank draws its own
    masks for its own samples."""

    ADD = 0xD6E8FEB86659FD93            # the stream's additive constant (mmgclip/augment.py's AugmentSeeds has another)

    def __init__(self):
        self._gen = self._epoch = None

    def reseed(self, seed=None):
        import torch
        from ..utils.global_utils import seed_epoch
        epoch, base = seed_epoch()
        if seed is None:
            seed = base if base is not None else torch.initial_seed()
        rank = int(os.environ.get("RANK", "0"))
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()
        # splitmix-style fold of (seed, rank) as in BertTower.reseed_dropout, with another additive constant: an unrelated stream
        mixed = (int(seed) * 0x9E3779B97F4A7C15 + (rank + 1) * 0xBF58476D1CE4E5B9 + self.ADD) & 0x7FFFFFFFFFFFFFFF
        self._gen = torch.Generator().manual_seed(mixed)
        self._epoch = epoch

    def draw(self):
        import torch
        from ..utils.global_utils import seed_epoch
        if self._gen is None or self._epoch != seed_epoch()[0]:
            self.reseed()
        return int(torch.randint(0, 2 ** 62, (1,), generator=self._gen).item())
