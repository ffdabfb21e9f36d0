"""Float64 / int64 reference, exact-data regime, derived intervals and an fp32 emulation (with mutations) for the retrieval ranks: the
kernel of csrc/retrieval_head.hip (mmg_retrieval_rows_rank) and the metrics of mmgclip/retrieval.py (RetrievalMetrics).

Imported by tests/test_retrieval_ref_cpu.py and tests/test_retrieval_cpu.py (no GPU) and by tests/test_retrieval_gpu.py (the kernel
against the same reference).  Everything here runs on the CPU.  The reference tree has no such metric: the independent statement the
reference below is pinned against is a dense, argsort-based ranking under the same tie convention (tests/test_retrieval_ref_cpu.py).

The operation (X [n_loc,D] local queries, Y [N,D] gallery, fp32):
    s_ij = <X_i,Y_j>;   positive: col_label None ? j == diag_off + i : col_label[j] == row_key[i]
    n_pos[i] = #positives;  best[i] = max of s_ij over them (-inf for none)
    n_gt[i] / n_eq[i] = #NEGATIVES with s_ij > best[i] / == best[i];   rank_i = 1 + n_gt + n_eq (ties count against the model)

Exact regime (exact_case): entries are integers in {-2..2} stored as fp32, so every s_ij is an integer of magnitude at most
4 D <= 4096 < 2^24: exact in fp32 under ANY summation order, and all four outputs compare by torch.equal.  Ties between a negative
and the best positive are planted (duplicated gallery rows) on top of the many that small integers give by themselves.

Gaussian regime (intervals): L2-normalised random rows.  An fp32 dot product on the f32 MFMA is within E_ij = Kd(D) u sum_d |x_d||y_d|
of the float64 one (u = 2^-24, Kd(n) = 2 n + 16: the project's convention, tests/sigmoid_ref.py).  The kernel's threshold is the
maximum of the positives' fp32 scores, so it lies in [b_lo, b_hi] = [max_p (s_ip - E_ip), max_p (s_ip + E_ip)].  A negative j is
SURELY above it when s_ij - E_ij > b_hi and POSSIBLY at or above it when s_ij + E_ij >= b_lo.  Hence for every query
    lo_i = #surely  <=  n_gt  <=  n_gt + n_eq  <=  #possibly = hi_i,
and where lo_i == hi_i both are that number and n_eq = 0.  No measured constant is involved.  A case may be used only when at most
1/8 of its rows have lo_i < hi_i (open_share; asserted on the reference alone), or a wrong count could hide in an open interval.

The emulation (emulate) is the kernel's arithmetic in fp32 torch on tiles padded as clip_tile.h pads them (rows >= n_loc and columns
>= N are clamped duplicates of the last valid one, never counted or written); TorchRetrievalBackend is `head._HipRetrievalBackend`
restated with it.  MUTATIONS break one thing at a time."""
import collections
import math
import types

import torch

from tests.sigmoid_ref import Kd, U, gaussian_case, hand_labels, positive_mask

# (n_loc, N, D, diag_off): the smallest shapes at which the tiling can go wrong - one pair; one partial tile; one tile and one row /
# column more; three row tiles at the widest D; one column more than a workgroup pass (4 waves x 32); the rows of a rank that is not
# the first; three tiles for some waves and a second, partial workgroup.
EXACT_SHAPES = ((1, 1, 32, 0), (31, 31, 32, 0), (33, 33, 64, 0), (65, 65, 1024, 0), (32, 129, 512, 0), (32, 96, 64, 64), (40, 300, 64, 0))
GAUSS_SHAPES = ((31, 31, 32, 0), (33, 33, 64, 0), (34, 35, 256, 0), (32, 96, 64, 64), (96, 300, 64, 0))
MODES = ("diagonal", "labels")
OPEN_CAP = 1.0 / 8.0
ABSENT_KEY = -7           # a query key no gallery label carries (labels are >= 0)


def keys_for(mode, n_loc, N, diag_off, absent_row=None):
    """(row_key, col_label): None, None on the diagonal; sigmoid_ref.hand_labels otherwise (a cluster across the tile seam, a
    singleton, runs of three).  `absent_row`: that query's key is one no gallery label carries."""
    if mode == "diagonal":
        return None, None
    col_label = hand_labels(N)
    row_key = col_label[diag_off:diag_off + n_loc].clone()
    if absent_row is not None:
        row_key[absent_row] = ABSENT_KEY
    return row_key, col_label


def reference(X, Y, pos):
    """float64 scores, int64 counts from fp32 X [n,D], Y [N,D] and the boolean positives [n,N]."""
    s = X.double() @ Y.double().t()
    ninf = torch.full_like(s, float("-inf"))
    best = torch.where(pos, s, ninf).max(dim=1).values
    r = types.SimpleNamespace(s=s, pos=pos, best=best, n_pos=pos.sum(1))
    r.n_gt = (~pos & (s > best[:, None])).sum(1)
    r.n_eq = (~pos & (s == best[:, None])).sum(1)
    r.rank = 1 + r.n_gt + r.n_eq
    return r


def intervals(X, Y, pos):
    """The reference plus, per query, [lo, hi] for n_gt and for n_gt + n_eq, and [b_lo, b_hi] for best (see the module docstring)."""
    r = reference(X, Y, pos)
    E = Kd(X.shape[1]) * U * (X.double().abs() @ Y.double().abs().t())
    ninf = torch.full_like(r.s, float("-inf"))
    r.b_lo = torch.where(pos, r.s - E, ninf).max(dim=1).values
    r.b_hi = torch.where(pos, r.s + E, ninf).max(dim=1).values
    r.lo = (~pos & (r.s - E > r.b_hi[:, None])).sum(1)
    r.hi = (~pos & (r.s + E >= r.b_lo[:, None])).sum(1)
    r.open_share = float((r.lo < r.hi).double().mean())
    return r


def interval_violations(r, best, n_pos, n_gt, n_eq):
    """Complaints about a kernel's (or emulation's) outputs against intervals(); empty = inside for EVERY row."""
    bad = []
    best, n_pos, n_gt, n_eq = best.double(), n_pos.long(), n_gt.long(), n_eq.long()
    if not torch.equal(n_pos, r.n_pos):
        bad.append("n_pos")
    if not bool(((best >= r.b_lo) & (best <= r.b_hi)).all()):
        bad.append(f"best outside its bar, rows {torch.nonzero((best < r.b_lo) | (best > r.b_hi)).flatten().tolist()}")
    if bool((n_eq < 0).any()):
        bad.append("n_eq < 0")
    for name, v in (("n_gt", n_gt), ("n_gt + n_eq", n_gt + n_eq)):
        out = (v < r.lo) | (v > r.hi)
        if bool(out.any()):
            bad.append(f"{name} outside [lo, hi], rows {torch.nonzero(out).flatten().tolist()}")
    point = r.lo == r.hi
    if not (torch.equal(n_gt[point], r.n_gt[point]) and torch.equal(n_eq[point], r.n_eq[point])):
        bad.append("a point interval is not the reference's count")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
def exact_case(n_loc, N, D, diag_off, seed=0):
    """Integer rows in {-2..2}.  The gallery is random with every seventh row a copy of the one before it (a planted tie whenever
    one of the two is a positive and the other is not); even queries are their diagonal partner plus noise in {-1,0,1} (clamped),
    so they rank near the top, odd queries are random and rank anywhere."""
    g = torch.Generator().manual_seed(1000 * N + D + seed)
    Y = torch.randint(-2, 3, (N, D), generator=g).float()
    j = torch.arange(N)
    dup = (j % 7 == 3) & (j > 0)
    Y[dup] = Y[j[dup] - 1]
    X = torch.randint(-2, 3, (n_loc, D), generator=g).float()
    near = (Y[diag_off:diag_off + n_loc] + torch.randint(-1, 2, (n_loc, D), generator=g).float()).clamp(-2, 2)
    even = torch.arange(n_loc) % 2 == 0
    X[even] = near[even]
    return X.contiguous(), Y.contiguous()


def exactness_violations(X, Y):
    """Preconditions of the exact regime, on the inputs alone: integer entries in [-2, 2] and D <= 1024, so |s_ij| <= 4096."""
    bad = []
    for name, t in (("X", X), ("Y", Y)):
        if not bool(((t == t.round()) & (t.abs() <= 2)).all()):
            bad.append(f"{name} is not integer in [-2, 2]")
    if X.shape[1] > 1024:
        bad.append("D > 1024")
    return bad


def exact_pairs(N, D, seed=0, dup_every=5):
    """An exact-regime validation set with planted duplicate texts: (img, txt [N,D] integer fp32, ids int64 [N,S], group int64 [N]).
    Report j is a copy of an earlier report's text when j % dup_every == dup_every - 1; `group` is the first index with that text
    and `ids` are token ids that are equal exactly when the texts are.  Images are their report plus noise (even j) or random."""
    g = torch.Generator().manual_seed(77 + seed)
    txt = torch.randint(-2, 3, (N, D), generator=g).float()
    group = torch.arange(N)
    for j in range(N):
        if j % dup_every == dup_every - 1:
            src = int(torch.randint(0, j, (1,), generator=g))
            group[j] = group[src]
            txt[j] = txt[src]
    first = txt[torch.unique(group)]
    assert torch.unique(first, dim=0).shape[0] == first.shape[0], "two different reports drew the same text"
    img = torch.randint(-2, 3, (N, D), generator=g).float()
    near = (txt + torch.randint(-1, 2, (N, D), generator=g).float()).clamp(-2, 2)
    even = torch.arange(N) % 2 == 0
    img[even] = near[even]
    ids = torch.zeros(N, 6, dtype=torch.int64)
    ids[:, 0], ids[:, 1], ids[:, 2], ids[:, 3] = 101, 1000 + group // 50, 1000 + group % 50, 102
    return img.contiguous(), txt.contiguous(), ids, group


# ---------------------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------------------
def metrics_from_ranks(name, rank, n_pos, n_eq, ks):
    """The flat metric dict of one direction from the per-query integers, in Python integers and exactly rounded sums."""
    rank, n_pos, n_eq = (t.tolist() for t in (rank, n_pos, n_eq))
    kept = sorted(r for r, p in zip(rank, n_pos) if p > 0)
    n = len(kept)
    out = {f"{name}_R@{k}": sum(r <= k for r in kept) / n for k in sorted(ks)}
    out[f"{name}_median_rank"] = (kept[(n - 1) // 2] + kept[n // 2]) / 2
    hist = collections.Counter(kept)
    out[f"{name}_mrr"] = math.fsum(h / r for r, h in hist.items()) / n        # (exactly rounded: the grouping cannot matter)
    out[f"{name}_ties"] = sum(1 for e, p in zip(n_eq, n_pos) if p > 0 and e > 0) / n
    out[f"{name}_n_queries"] = n
    out[f"{name}_no_positive"] = len(rank) - n
    return out


def reference_metrics(img, txt, labels=None, ks=(1, 5, 10)):
    """The metrics of the UNSHARDED set in float64 / int64: i2t ranks images against all texts, t2i the reverse; labels None = the
    diagonal, else report j is a positive of query i when labels[j] == labels[i]."""
    N = img.shape[0]
    pos = positive_mask(N, N, 0, labels, labels)
    out = {}
    for name, x, y in (("i2t", img, txt), ("t2i", txt, img)):
        r = reference(x, y, pos)
        out.update(metrics_from_ranks(name, r.rank, r.n_pos, r.n_eq, ks))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# emulation of the kernel (fp32 torch) and its mutations
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("ge_for_gt", "pos_as_neg", "pad_col", "no_diag_off", "label_vs_index", "first_pos", "pad_row")


def _pad_to(t, rows):
    if t.shape[0] == rows:
        return t
    return torch.cat([t, t[-1:].expand(rows - t.shape[0], *t.shape[1:])])


def emulate(X, Y, row_key=None, col_label=None, diag_off=0, mut=None):
    """-> best fp32 [n], n_pos, n_gt, n_eq int32 [n], computed on padded tiles."""
    assert mut is None or mut in MUTATIONS, mut
    n, N = X.shape[0], Y.shape[0]
    np_, Np = 32 * math.ceil(n / 32), 32 * math.ceil(N / 32)
    s = _pad_to(X.float(), np_) @ _pad_to(Y.float(), Np).t()
    ig, jg = torch.arange(np_), torch.arange(Np)
    off = 0 if mut == "no_diag_off" else diag_off
    if col_label is None:
        pos = jg[None, :] == (off + ig)[:, None]
    else:
        rk = (diag_off + ig) if mut == "label_vs_index" else _pad_to(row_key, np_)
        pos = _pad_to(col_label, Np)[None, :] == rk[:, None]
    valid = torch.ones(np_, Np, dtype=torch.bool) if mut == "pad_col" else (jg < N)[None, :].expand(np_, Np)
    pos = pos & valid
    n_pos = pos.sum(1)
    ninf = torch.full_like(s, float("-inf"))
    if mut == "first_pos":
        first = torch.where(pos, jg[None, :].expand(np_, Np), torch.full((np_, Np), Np)).min(dim=1).values
        best = torch.where(n_pos > 0, s[ig, first.clamp(max=Np - 1)], ninf[:, 0])
    else:
        best = torch.where(pos, s, ninf).max(dim=1).values
    neg = valid if mut == "pos_as_neg" else (valid & ~pos)
    n_eq = (neg & (s == best[:, None])).sum(1)
    n_gt = (neg & ((s >= best[:, None]) if mut == "ge_for_gt" else (s > best[:, None]))).sum(1)
    rows = np_ if mut == "pad_row" else n
    return best[:rows].contiguous(), n_pos[:rows].int(), n_gt[:rows].int(), n_eq[:rows].int()


class TorchRetrievalBackend:
    """`head._HipRetrievalBackend` restated with emulate(): what the CPU / gloo tests install in its place."""

    @staticmethod
    def rank(x_loc, y_all, row_key, col_label, diag_off):
        return emulate(x_loc, y_all, row_key, col_label, diag_off)
