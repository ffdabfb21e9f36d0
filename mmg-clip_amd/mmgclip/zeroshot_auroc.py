"""Zero-shot prompt AUROC on the device: exact pair counts and seeded bootstrap intervals, global over a data-parallel run, from the
i8 matrix-core kernel of csrc/auroc_head.hip (`head._HipAurocBackend`).  Nothing here runs unless `experiments.config.zeroshot_auroc`
is set (ClassifierExperiment.validate) or `Evaluator.zeroshot_label_prompt(ci="device")` is asked for.

The formula.  With positive scores s+_i, negative scores s-_j and integer resampling weights,
    AUROC_b = U2_b / (2 W+_b W-_b),   U2_b = sum_i sum_j w+[b,i] w-[b,j] g(s+_i, s-_j),   g = 2 [s+ > s-] + [s+ == s-],
W+_b / W-_b the weight totals of replicate b.  A bootstrap replicate is that sum with the resample's multiplicities as weights - equal
to sklearn's roc_auc_score on the resampled arrays, ties included (tests/test_auroc_ref_cpu.py) - and the point estimate is the
replicate whose weights are all 1.  The kernel returns U2_b as an integer; the division is ONE Python integer division per replicate,
which is correctly rounded, so every figure is the same whoever computes it.

The draws.  Replicate b draws N samples (N the GLOBAL sample count): draw t' lands on idx = (u * N) >> 32 with
u = mmg_drop_bits(t', mmg_drop_key_bh(mmg_drop_key(seed, 0x200), b)), the hash of csrc/dropout.h; the multiply-high's bias is below
N / 2^32 per value.  The weight of sample t is how often it was drawn; the same resample serves every class and every task of N
samples, so a task's macro mean has an interval of its own.  A count above 127 (int8) raises; real draws stay near 10.

Classes.  Column c's positives are `targets == class_values[c]`; every other sample is a negative, as validate() has it: BI-RADS
`unknown` = -1 is a negative of every class that is not -1.  A class without a positive or without a negative has auc = nan and
launches nothing; replicates in which a class has no positive or no negative weight are left out of its interval (the reference's
`len(unique) == 2` test, evaluator.py:135), and out of the macro interval when that happens to any class the macro mean is taken over.
The interval is the reference's `calculate_ci`: sorted index int(0.025 len) and int(0.975 len); `ci_mean` is math.fsum / len.

A data-parallel run.  Scores and targets are gathered (uneven shards as `RetrievalMetrics._gather` handles them); every rank takes
its LOCAL positives against the GLOBAL negatives with weights indexed by the global sample number; the per-replicate U2 of all tasks
go through ONE int64 all-reduce per `compute()`.  W+_b is a function of the gathered targets, the same on every rank.  The dict is
identical on every rank and equal to the unsharded one.

Replicates are processed in chunks so that the transient weights stay under `max_weight_bytes`; the result does not depend on the
chunking.  Per replicate and N padded to 16 columns (`replicates_per_chunk`): the multiplicities themselves (N bytes), then either the
int32 widening torch makes of the smaller of a class's two sides to sum it (at most 2 N; the other side's total is N minus it, because
a replicate's weights sum to N) or the positive and negative columns gathered for the kernel (N + 32) with its int64 partials (N / 4):
4 N + 32 bytes bounds both."""
import math

import torch

from . import head
from .retrieval import RetrievalMetrics

NAN = math.nan


def parse_config(node):
    """`experiments.config.zeroshot_auroc` -> the keyword arguments of ZeroShotAUROC, or None when the key is null / absent."""
    if node is None:
        return None
    if not isinstance(node, dict):
        raise ValueError(f"experiments.config.zeroshot_auroc must be null or a mapping with n_bootstrap / seed, got {node!r}")
    unknown = set(node) - {"n_bootstrap", "seed"}
    if unknown:
        raise ValueError(f"experiments.config.zeroshot_auroc: unknown keys {sorted(unknown)}")
    kw = {k: node[k] for k in ("n_bootstrap", "seed") if node.get(k) is not None}
    ZeroShotAUROC(**kw)          # validates
    return kw


def _pad16(w):
    """[B, m] int8 -> contiguous [B, ceil16(m)] with zeros in the padding (at least 16 wide)."""
    pad = max(16, (w.shape[1] + 15) // 16 * 16) - w.shape[1]
    return (torch.nn.functional.pad(w, (0, pad)) if pad else w).contiguous()


def replicates_per_chunk(N, max_weight_bytes):
    """Replicates taken at a time so that the transient weights of N samples stay under `max_weight_bytes`: at least one, and at
    most the 65535 that one `mmg_bootstrap_weights` call takes."""
    return min(65535, max(1, max_weight_bytes // (4 * ((N + 15) // 16 * 16) + 32)))


def interval(values):
    """(ci_mean, ci_lower, ci_upper, n_valid) of the replicates' values by the reference's calculate_ci rule."""
    if not values:
        return NAN, NAN, NAN, 0
    s = sorted(values)
    return math.fsum(values) / len(values), s[int(0.025 * len(s))], s[int(0.975 * len(s))], len(s)


class ZeroShotAUROC:
    def __init__(self, n_bootstrap=1000, seed=0, comm=None, max_weight_bytes=64 << 20):
        for name, v in (("n_bootstrap", n_bootstrap), ("seed", seed)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
        if seed >= 2 ** 64:
            raise ValueError(f"seed must fit 64 bits, got {seed!r}")
        if isinstance(max_weight_bytes, bool) or not isinstance(max_weight_bytes, int) or max_weight_bytes < 1:
            raise ValueError(f"max_weight_bytes must be a positive integer, got {max_weight_bytes!r}")
        self.n_bootstrap, self.seed, self.comm, self.max_weight_bytes = n_bootstrap, seed, comm, max_weight_bytes
        self._exchange = RetrievalMetrics(comm=comm)          # its shard counts and uneven all-gather, by composition
        self.reset()

    def reset(self):
        self._tasks = {}

    @property
    def has_data(self):
        """Whether any batch was fed on THIS rank.  `compute()` is collective in a data-parallel run: every rank has to call it,
        with the same tasks fed, or the others wait in its gathers - a rank with an empty validation loader cannot take part
        (`RetrievalMetrics` has the same limit)."""
        return bool(self._tasks)

    def update(self, name, scores, targets, class_values):
        """One validation batch of task `name`: the [n,k] prompt scores, the [n] integer targets and the k class values (column c
        scores class `class_values[c]`).  Kept on the device, fp32 / int64; nothing is computed here."""
        scores = scores.detach().float()
        targets = torch.as_tensor(targets).detach().to(device=scores.device, dtype=torch.int64)
        class_values = [int(v) for v in class_values]
        if scores.ndim != 2 or targets.ndim != 1 or targets.shape[0] != scores.shape[0] or len(class_values) != scores.shape[1]:
            raise ValueError(f"scores must be [n,k] with n targets and k class values, got {tuple(scores.shape)}, {tuple(targets.shape)}, "
                             f"{len(class_values)} class values")
        if len(set(class_values)) != len(class_values):
            raise ValueError(f"class_values must be distinct, got {class_values}")
        task = self._tasks.setdefault(name, dict(class_values=class_values, scores=[], targets=[]))
        if task["class_values"] != class_values:
            raise ValueError(f"task {name!r} was fed with class values {task['class_values']} before, now {class_values}")
        task["scores"].append(scores.clone())
        task["targets"].append(targets.clone())

    # ---- the device part: U2 of the local positives, W+ of the global ones --------------------------------------------------------
    def _task_counts(self, task):
        """-> (u2 [k, 1+B] int64 of the LOCAL positives, wp [k, 1+B] int64 GLOBAL, N, overflow flag); column 0 is the point estimate.
        The host learns the class sizes here (`nonzero` synchronises, a few times per class), and the point estimate is a pairs
        launch of its own per class: fine once per validation epoch, not a path to put in a training step."""
        be = head._HipAurocBackend
        ex = self._exchange
        scores, targets = torch.cat(task["scores"]).contiguous(), torch.cat(task["targets"]).contiguous()
        n_loc, dev, B = scores.shape[0], scores.device, self.n_bootstrap
        counts = ex._shard_counts(n_loc, dev)
        off, N = sum(counts[:self.comm.rank if ex._sharded else 0]), sum(counts)
        scores_all, targets_all = ex._gather(scores, counts), ex._gather(targets, counts)
        k = scores.shape[1]
        u2 = torch.zeros((k, 1 + B), dtype=torch.int64, device=dev)
        wp = torch.zeros((k, 1 + B), dtype=torch.int64, device=dev)
        classes = []
        for c, cv in enumerate(task["class_values"]):
            pos_all = targets_all == cv
            glob = torch.nonzero(pos_all).flatten()
            neg = torch.nonzero(~pos_all).flatten()
            wp[c, 0] = glob.numel()
            if glob.numel() == 0 or neg.numel() == 0:
                continue                                   # undefined: nan on the host, nothing launched
            loc = torch.nonzero(targets == cv).flatten()
            s_pos, s_neg = scores[loc, c].contiguous(), scores_all[neg, c].contiguous()
            classes.append((c, glob, loc + off, neg, s_pos, s_neg))
            if loc.numel():
                ones_p = _pad16(torch.ones((1, loc.numel()), dtype=torch.int8, device=dev))
                ones_n = _pad16(torch.ones((1, neg.numel()), dtype=torch.int8, device=dev))
                u2[c, 0] = be.pairs(s_pos, s_neg, ones_p, ones_n, neg_total=neg.numel())[0]
        if 2 * N >= 2 ** 31:
            raise ValueError(f"{N} samples: a replicate's weights sum to N, and 2 N must stay below 2^31 (int32 accumulators)")
        lightest = torch.zeros((), dtype=torch.int8, device=dev)          # the smallest weight seen: negative = a count above 127
        chunk = replicates_per_chunk(N, self.max_weight_bytes)
        for b0 in range(0, B if classes else 0, chunk):
            bc = min(chunk, B - b0)
            w = be.bootstrap_weights(self.seed, N, b0, bc, dev)
            lightest = torch.minimum(lightest, w.min())
            cols = slice(1 + b0, 1 + b0 + bc)
            for c, glob, loc_g, neg, s_pos, s_neg in classes:
                # W+ from the smaller side (torch widens what it sums; a replicate's weights sum to N)
                if glob.numel() <= neg.numel():
                    wp[c, cols] = w.index_select(1, glob).sum(dim=1, dtype=torch.int32)
                else:
                    wp[c, cols] = N - w.index_select(1, neg).sum(dim=1, dtype=torch.int32)
                if loc_g.numel():
                    u2[c, cols] = be.pairs(s_pos, s_neg, _pad16(w.index_select(1, loc_g)), _pad16(w.index_select(1, neg)), neg_total=N)
        return u2, wp, N, lightest < 0

    def compute(self):
        """{task: {"auc", "n_classes", ["ci_mean", "ci_lower", "ci_upper", "n_valid"], "classes": {class value: {"auc", "n_pos",
        "n_neg", [the same four]}}}}: plain Python numbers, identical on every rank.  The task's own figures are the macro mean over
        the classes where AUROC is defined."""
        if not self._tasks:
            raise ValueError("ZeroShotAUROC.compute() before any update() on this rank")
        names = sorted(self._tasks)
        parts = [self._task_counts(self._tasks[n]) for n in names]
        if bool(torch.stack([p[3] for p in parts]).any()):
            raise OverflowError("a bootstrap replicate drew one sample more than 127 times: the int8 weights cannot hold it")
        flat = torch.cat([p[0].flatten() for p in parts])
        if self._exchange._sharded:
            flat = self.comm.all_reduce_sum(flat)
        flat, out, at = flat.tolist(), {}, 0
        for name, (u2, wp, N, _) in zip(names, parts):
            k, width = u2.shape
            rows = [flat[at + c * width: at + (c + 1) * width] for c in range(k)]
            at += k * width
            out[name] = self._from_counts(self._tasks[name]["class_values"], rows, wp.tolist(), N)
        return out

    # ---- the host part: integers in, correctly rounded figures out -----------------------------------------------------------------
    def _from_counts(self, class_values, u2, wp, N):
        B = self.n_bootstrap
        classes, defined = {}, []
        for cv, u, w in zip(class_values, u2, wp):
            P, Nn = w[0], N - w[0]
            ok = P > 0 and Nn > 0
            entry = {"auc": u[0] / (2 * P * Nn) if ok else NAN, "n_pos": P, "n_neg": Nn}
            reps = [u[b] / (2 * w[b] * (N - w[b])) if ok and 0 < w[b] < N else None for b in range(1, 1 + B)]
            if B:
                entry.update(zip(("ci_mean", "ci_lower", "ci_upper", "n_valid"), interval([v for v in reps if v is not None])))
            classes[cv] = entry
            if ok:
                defined.append((entry["auc"], reps))
        task = {"auc": math.fsum(a for a, _ in defined) / len(defined) if defined else NAN, "n_classes": len(defined)}
        if B:
            macro = []
            for b in range(B if defined else 0):          # the same resample for every class: a replicate counts when all are defined
                vals = [reps[b] for _, reps in defined]
                if all(v is not None for v in vals):
                    macro.append(math.fsum(vals) / len(vals))
            task.update(zip(("ci_mean", "ci_lower", "ci_upper", "n_valid"), interval(macro)))
        task["classes"] = classes
        return task
