"""TEST INFRASTRUCTURE - the int64 / float64 reference of the zero-shot AUROC with bootstrap replicates (mmgclip/zeroshot_auroc.py,
csrc/auroc_head.hip), and a torch int64 emulation of the two kernels for the CPU tests.

Two independent statements of the same arithmetic:
  * the REFERENCE, numpy: the draws of csrc/dropout.h's hash restated (as mmgclip/augment.py restates its draws), the weights as their
    bincount, a dense G = 2 [s+ > s-] + [s+ == s-] in int64, U2_b = w+_b G w-_b, and the dict of `ZeroShotAUROC.compute()` from Python
    integers (one correctly rounded division per replicate; the interval by the reference's calculate_ci rule);
  * the EMULATION, torch: `TorchAurocBackend` stands in for `head._HipAurocBackend` (same signatures, same int8 layout with zero
    padding to a multiple of 16).  `emulation(mutation)` builds deliberately wrong variants; tests/test_auroc_ref_cpu.py shows that
    every one of them fails an exact case."""
import math

import numpy as np
import torch

from oracle.dropout_oracle import drop_key, fmix32

SITE_BOOTSTRAP = 0x200
_M32 = np.uint64(0xFFFFFFFF)
MUTATIONS = ("ge_for_gt", "tie_counts_0", "tie_counts_2", "weights_transposed", "padded_column_counted", "positive_weights_ignored",
             "one_class_replicate_kept", "modulo_draw")


# ---- the draws ----------------------------------------------------------------------------------------------------------------------
def draws(seed, n, b, modulo=False):
    """The n sample indices replicate b draws: idx = (u * n) >> 32, u = drop_bits(t', key_bh(drop_key(seed, SITE_BOOTSTRAP), b))."""
    key_b = fmix32((np.uint64(drop_key(seed, SITE_BOOTSTRAP)) + np.uint64(b) * np.uint64(0xB5297A4D)) & _M32)
    u = fmix32((np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + key_b) & _M32)
    return (u % np.uint64(n) if modulo else (u * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def weights(seed, n, b0, B, modulo=False):
    """int64 [B, n]: how many of replicate b's draws landed on sample t, b = b0 .. b0+B-1."""
    return np.stack([np.bincount(draws(seed, n, b, modulo), minlength=n) for b in range(b0, b0 + B)]).astype(np.int64)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def g_matrix(s_pos, s_neg):
    sp, sn = np.asarray(s_pos, dtype=np.float32)[:, None], np.asarray(s_neg, dtype=np.float32)[None, :]
    return 2 * (sp > sn).astype(np.int64) + (sp == sn).astype(np.int64)


def u2(s_pos, s_neg, w_pos, w_neg):
    """int64 [B]: sum_ij w_pos[b,i] w_neg[b,j] g(s_pos[i], s_neg[j]) for weights [B,P] / [B,Nn]."""
    G = g_matrix(s_pos, s_neg)
    return np.einsum("bi,ij,bj->b", np.asarray(w_pos, dtype=np.int64), G, np.asarray(w_neg, dtype=np.int64))


def calculate_ci(scores):
    """mmgclip/evaluator.py's rule, with an exactly rounded mean."""
    if not scores:
        return math.nan, math.nan, math.nan, 0
    s = np.sort(np.asarray(scores, dtype=np.float64))
    return math.fsum(scores) / len(scores), float(s[int(0.025 * len(s))]), float(s[int(0.975 * len(s))]), len(scores)


def replicate_aucs(scores, positive, seed, B, keep_one_class=False, w=None):
    """AUROC of every replicate (None where it has one class only) of one score column against a boolean `positive`."""
    scores, positive = np.asarray(scores, dtype=np.float32), np.asarray(positive, dtype=bool)
    n = scores.shape[0]
    w = weights(seed, n, 0, B) if w is None else w
    U = u2(scores[positive], scores[~positive], w[:, positive], w[:, ~positive])
    out = []
    for b in range(B):
        wp = int(w[b, positive].sum())
        wn = int(w[b].sum()) - wp
        if wp > 0 and wn > 0:
            out.append(int(U[b]) / (2 * wp * wn))
        else:
            out.append(0.5 if keep_one_class else None)
    return out


def reference(tasks, n_bootstrap, seed):
    """The dict of ZeroShotAUROC.compute() for tasks = {name: (scores [n,k], targets [n], class_values)}, unsharded."""
    out = {}
    for name in sorted(tasks):
        scores, targets, class_values = tasks[name]
        scores, targets = np.asarray(scores, dtype=np.float32), np.asarray(targets, dtype=np.int64)
        n = scores.shape[0]
        w = weights(seed, n, 0, n_bootstrap) if n_bootstrap else np.zeros((0, n), dtype=np.int64)
        classes, defined = {}, []
        for c, cv in enumerate(class_values):
            pos = targets == cv
            P, Nn = int(pos.sum()), int((~pos).sum())
            ok = P > 0 and Nn > 0
            point = int(u2(scores[pos, c], scores[~pos, c], np.ones((1, P), np.int64), np.ones((1, Nn), np.int64))[0]) / (2 * P * Nn) if ok else math.nan
            entry = {"auc": point, "n_pos": P, "n_neg": Nn}
            reps = replicate_aucs(scores[:, c], pos, seed, n_bootstrap, w=w) if ok else [None] * n_bootstrap
            if n_bootstrap:
                entry.update(zip(("ci_mean", "ci_lower", "ci_upper", "n_valid"), calculate_ci([v for v in reps if v is not None])))
            classes[int(cv)] = entry
            if ok:
                defined.append((point, reps))
        task = {"auc": math.fsum(a for a, _ in defined) / len(defined) if defined else math.nan, "n_classes": len(defined)}
        if n_bootstrap:
            macro = [math.fsum(r[b] for _, r in defined) / len(defined) for b in range(n_bootstrap if defined else 0)
                     if all(r[b] is not None for _, r in defined)]
            task.update(zip(("ci_mean", "ci_lower", "ci_upper", "n_valid"), calculate_ci(macro)))
        task["classes"] = classes
        out[name] = task
    return out


def same(a, b):
    """`==` on the nested dicts with nan equal to nan (a class without positives has nan figures on both sides)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return type(a) is type(b) and a == b


# ---- the emulation ------------------------------------------------------------------------------------------------------------------
def emulation(mutation=None, patched_draw=None):
    """A stand-in for head._HipAurocBackend in torch int64 (CPU or device tensors).  `mutation`: one of MUTATIONS or None;
    `patched_draw(seed, n, b) -> indices` replaces the draw (the overflow test)."""
    assert mutation is None or mutation in MUTATIONS, mutation

    class TorchBackend:
        @staticmethod
        def bootstrap_weights(seed, n, b0, B, device=None):
            if patched_draw is not None:
                w = np.stack([np.bincount(patched_draw(seed, n, b), minlength=n) for b in range(b0, b0 + B)])
            else:
                w = weights(seed, n, b0, B, modulo=mutation == "modulo_draw")
            w = np.where(w > 127, -128, w)
            out = torch.zeros((B, (n + 15) // 16 * 16), dtype=torch.int8, device=device)
            out[:, :n] = torch.from_numpy(w).to(torch.int8)
            return out

        @staticmethod
        def pairs(s_pos, s_neg, w_pos, w_neg, neg_total=None):
            P, Nn, B = s_pos.shape[0], s_neg.shape[0], w_neg.shape[0]
            assert neg_total is None or int(w_neg.sum(dim=1, dtype=torch.int64).max()) <= neg_total
            assert w_pos.dtype == torch.int8 and w_neg.dtype == torch.int8 and w_pos.shape[0] == B
            assert w_pos.shape[1] % 16 == 0 and w_neg.shape[1] % 16 == 0 and w_pos.shape[1] >= P and w_neg.shape[1] >= Nn
            assert 2 * int(w_neg.sum(dim=1, dtype=torch.int64).max()) < 2 ** 31
            sp, sn = s_pos.float()[:, None], s_neg.float()[None, :]
            wn = w_neg
            if mutation == "weights_transposed":           # the [B][ld] bytes read as [ld][B]
                wn = w_neg.reshape(w_neg.shape[1], B).t()
            if mutation == "padded_column_counted":        # the K padding taken for samples: the last score again, with weight 1
                pad = w_neg.shape[1] - Nn
                sn = torch.cat([sn, sn[:, -1:].expand(1, pad)], dim=1)
                wn = torch.cat([wn[:, :Nn], torch.ones((B, pad), dtype=torch.int8, device=wn.device)], dim=1)
                Nn += pad
            gt, eq = (sp > sn).to(torch.int64), (sp == sn).to(torch.int64)
            G = {None: 2 * gt + eq, "ge_for_gt": 2 * (gt + eq) + eq, "tie_counts_0": 2 * gt, "tie_counts_2": 2 * (gt + eq)}.get(mutation, 2 * gt + eq)
            wp = w_pos[:, :P].to(torch.int64)
            if mutation == "positive_weights_ignored":
                wp = torch.ones_like(wp)
            return ((wp @ G) * wn[:, :Nn].to(torch.int64)).sum(dim=1)

    return TorchBackend


TorchAurocBackend = emulation()


def emulated_replicate_aucs(backend, scores, positive, seed, B, keep_one_class=False):
    """`replicate_aucs` through a backend: weights, the gather of the positive / negative columns, pairs, the division."""
    scores = torch.as_tensor(np.asarray(scores, dtype=np.float32))
    positive = torch.as_tensor(np.asarray(positive, dtype=bool))
    n = scores.shape[0]
    w = backend.bootstrap_weights(seed, n, 0, B)
    if bool((w < 0).any()):
        raise OverflowError("a count above 127")
    pad = lambda t: torch.nn.functional.pad(t, (0, -t.shape[1] % 16)).contiguous()          # noqa: E731
    pos, neg = torch.nonzero(positive).flatten(), torch.nonzero(~positive).flatten()
    U = backend.pairs(scores[pos], scores[neg], pad(w.index_select(1, pos)), pad(w.index_select(1, neg))).tolist()
    wp = w.index_select(1, pos).sum(dim=1, dtype=torch.int64).tolist()
    out = []
    for b in range(B):
        wn = n - wp[b]
        if wp[b] > 0 and wn > 0:
            out.append(U[b] / (2 * wp[b] * wn))
        else:
            out.append(0.5 if keep_one_class else None)
    return out


# ---- shared cases -------------------------------------------------------------------------------------------------------------------
def tie_scores(n, seed):
    """fp32 integers in -6..6 (ties are plentiful), zeros of both signs among them."""
    g = np.random.default_rng(seed)
    s = g.integers(-6, 7, n).astype(np.float32)
    zero = np.flatnonzero(s == 0)
    s[zero[::2]] = np.float32(-0.0)
    return s


def example_tasks(n=150, seed=3):
    """A binary task and a 4-class task on the same n samples: scores with ties in the first, normal in the second; the 4-class
    targets include -1 ("unknown"), a negative of every class."""
    g = np.random.default_rng(seed)
    y = (g.random(n) < 0.3).astype(np.int64)
    malig = (tie_scores(n, seed + 1) + 2 * y).astype(np.float32)[:, None]
    t4 = g.integers(-1, 4, n).astype(np.int64)
    shapes = g.standard_normal((n, 4)).astype(np.float32)
    shapes[np.arange(n)[t4 >= 0], t4[t4 >= 0]] += 1.0
    return {"malig": (malig, y, [1]), "shapes": (shapes, t4, [0, 1, 2, 3])}
