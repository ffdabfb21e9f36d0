"""Float64 reference, exact-data regime, derived intervals and an fp32 emulation (with mutations) for the nearest-neighbour search: the
kernel of csrc/topk_head.hip (mmg_topk_rows) and the index of mmgclip/search.py (merge_topk, EmbeddingIndex).

Imported by tests/test_topk_ref_cpu.py and tests/test_topk_cpu.py (no GPU) and by tests/test_topk_gpu.py (the kernel against the same
reference).  Everything here runs on the CPU.  The reference tree has no search: the independent statement the reference below is
pinned against is a dense per-row argsort written in tests/test_topk_ref_cpu.py.

The operation (X [n_loc,D] local queries, Y [N,D] gallery chunk, fp32):
    s_ij = <X_i,Y_j>;  column j has the global index J = j_base + j
    excluded: none | J == diag_off + i | col_label[j] == row_key[i]
    row i receives its k best admissible columns under the TOTAL order (score descending, then J ascending), padded with -inf / -1;
    with `accumulate` the lists already in the buffers (over other columns) take part.

Exact regime (exact_case): entries are integers in {-2..2} stored as fp32, so every s_ij is an integer of magnitude at most
4 D <= 4096 < 2^24: exact in fp32 under ANY summation order, so scores and indices compare by torch.equal.  Every seventh gallery row
is a copy of its predecessor and small integers tie by themselves: ties are everywhere, and only the index tie-break decides them.

Gaussian regime (intervals): L2-normalised random rows.  An fp32 dot product on the f32 MFMA is within E_ij = Kd(D) u sum_d |x_d||y_d|
of the float64 one (u = 2^-24, Kd(n) = 2 n + 16: the project's convention, tests/sigmoid_ref.py).  Whatever the fp32 scores are inside
their bars, admissible column j is SURELY IN the top k when fewer than k other admissible j' have s_ij' + E_ij' >= s_ij - E_ij, and
SURELY OUT when at least k admissible j' have s_ij' - E_ij' > s_ij + E_ij.  A row is OPEN when some admissible column is neither.  No
measured constant is involved.  A case may be used only when at most 1/8 of its rows are open (open_share; asserted on the reference
alone), or a wrong selection could hide among undecided columns.  Where, on top, every gap between consecutive float64 scores of a
row's top k+1 exceeds the sum of their two bars, the fp32 order of those columns is the float64 one and the index row must be the
reference's.

The emulation (emulate) is the kernel's arithmetic in fp32 torch on tiles padded as clip_tile.h pads them (rows >= n_loc and columns
>= N are clamped duplicates of the last valid one, never admitted or written), with the kernel's structure restated: one list per
wave (tiles jt = wave mod 4) fed by both lane halves (tile columns with bit 2 clear / set), wave 0's list seeded with the incoming
list under `accumulate`, a four-way merge.  TorchTopKBackend is `head._HipTopKBackend` restated with it.  MUTATIONS break one thing at
a time."""
import math
import types

import torch

from tests.sigmoid_ref import Kd, U, gaussian_case, hand_labels, positive_mask

# (n_loc, N, D, diag_off, k): the smallest shapes at which this tiling can go wrong - the smallest launch; k > N (padding); a short
# launch; a second workgroup of one row with k about N; one column beyond a four-wave pass; the rows of a later rank; three tiles for
# some waves and a partial workgroup; the largest LDS plan that must be supported; the widest D at its guaranteed k.
EXACT_SHAPES = ((1, 1, 32, 0, 1), (3, 5, 32, 0, 8), (31, 31, 32, 0, 5), (33, 33, 64, 0, 32), (32, 129, 512, 0, 10), (32, 96, 64, 64, 4),
                (40, 300, 64, 0, 32), (8, 70, 768, 0, 32), (65, 65, 1024, 0, 16))
GAUSS_SHAPES = ((31, 31, 32, 0, 5), (33, 33, 64, 0, 32), (34, 35, 256, 0, 8), (32, 96, 64, 64, 4), (32, 129, 512, 0, 10), (96, 300, 64, 0, 32))
MODES = ("none", "diagonal", "labels")
EXCLUDE = {"none": 0, "diagonal": 1, "labels": 2}
OPEN_CAP = 1.0 / 8.0
ABSENT_KEY = -7           # a query key no gallery label carries (labels are >= 0)
ABSENT_CASE = ((40, 300, 64, 0, 32), 5)          # the labelled case that carries a query whose key matches nothing
MAX_K = 32
LDS_LIMIT = 163840
NINF = float("-inf")
_LAST = torch.iinfo(torch.int64).max


def lds_bytes(D, k):
    """The launch's dynamic LDS: the staged rows 32 (D+4) 4 and the lists 4 x 32 x k x 8."""
    return 32 * (D + 4) * 4 + 4 * 32 * k * 8


def supported(D, k):
    return D % 32 == 0 and 32 <= D <= 1024 and 1 <= k <= MAX_K and lds_bytes(D, k) <= LDS_LIMIT


def keys_for(mode, n_loc, N, diag_off, absent_row=None):
    """(row_key, col_label): None, None unless mode is `labels`; sigmoid_ref.hand_labels otherwise (a cluster across the tile seam, a
    singleton, runs of three).  `absent_row`: that query's key is one no gallery label carries."""
    if mode != "labels":
        return None, None
    col_label = hand_labels(N)
    row_key = col_label[(diag_off + torch.arange(n_loc)).clamp(max=N - 1)].clone()
    if absent_row is not None:
        row_key[absent_row] = ABSENT_KEY
    return row_key, col_label


def excluded_mask(mode, n_loc, N, diag_off, row_key, col_label):
    if mode == "none":
        return torch.zeros(n_loc, N, dtype=torch.bool)
    if mode == "diagonal":
        return positive_mask(n_loc, N, diag_off)
    return positive_mask(n_loc, N, diag_off, row_key, col_label)


def case(shape, mode, regime):
    """-> X, Y, row_key, col_label, excluded [n,N] of a test case."""
    n, N, D, off, _ = shape
    X, Y = exact_case(n, N, D, off) if regime == "exact" else gaussian_case(n, N, D, 0)
    absent = ABSENT_CASE[1] if (mode == "labels" and shape == ABSENT_CASE[0]) else None
    key, lab = keys_for(mode, n, N, off, absent)
    return X, Y, key, lab, excluded_mask(mode, n, N, off, key, lab)


def three_cuts(N):
    """Three uneven, non-empty column chunks of N (fewer when N < 3): [(a, b), ...]."""
    c1 = max(1, N * 3 // 7)
    c2 = max(c1 + 1, N * 5 // 7)
    edges = sorted({0, min(c1, N), min(c2, N), N})
    return list(zip(edges[:-1], edges[1:]))


# ---------------------------------------------------------------------------------------------------------------------------------
# reference and intervals
# ---------------------------------------------------------------------------------------------------------------------------------
def reference(X, Y, k, excluded, j_base=0):
    """float64 scores of fp32 X [n,D], Y [N,D]; per row a stable descending sort (the index breaks ties), the first k admissible
    columns, padded with -inf / -1.  -> .s [n,N], .scores float64 [n,k], .indices int64 [n,k] (global: j_base + j), .n_adm [n]."""
    s = X.double() @ Y.double().t()
    n, N = s.shape
    masked = torch.where(excluded, torch.full_like(s, NINF), s)          # finite scores stand before every excluded column
    order = torch.sort(masked, dim=1, descending=True, stable=True).indices[:, :k]
    scores, indices = masked.gather(1, order), order + j_base
    if N < k:
        scores = torch.cat([scores, scores.new_full((n, k - N), NINF)], dim=1)
        indices = torch.cat([indices, indices.new_full((n, k - N), -1)], dim=1)
    n_adm = (~excluded).sum(1)
    pad = torch.arange(k)[None, :] >= n_adm[:, None]
    scores = torch.where(pad, torch.full_like(scores, NINF), scores)
    indices = torch.where(pad, torch.full_like(indices, -1), indices)
    return types.SimpleNamespace(s=s, scores=scores, indices=indices, n_adm=n_adm, excluded=excluded, k=k, j_base=j_base)


def intervals(X, Y, k, excluded, j_base=0):
    """The reference plus E [n,N], the surely-in / surely-out columns, the open rows and the rows whose order is decided."""
    r = reference(X, Y, k, excluded, j_base)
    n, N = r.s.shape
    r.E = Kd(X.shape[1]) * U * (X.double().abs() @ Y.double().abs().t())
    adm = ~excluded
    hi = torch.where(adm, r.s + r.E, torch.full_like(r.s, NINF))          # an excluded column is never above anything
    lo = torch.where(adm, r.s - r.E, torch.full_like(r.s, NINF))
    # possibly[i,j] = # admissible j' != j with hi[i,j'] >= lo[i,j];  surely[i,j] = # admissible j' with lo[i,j'] > hi[i,j]
    possibly = (hi[:, None, :] >= lo[:, :, None]).sum(2) - adm.long()     # (j itself always satisfies hi >= lo when admissible)
    surely = (lo[:, None, :] > hi[:, :, None]).sum(2)
    r.sure_in = adm & (possibly < k)
    r.sure_out = adm & (surely >= k)
    r.open_rows = (adm & ~r.sure_in & ~r.sure_out).any(1)
    r.open_share = float(r.open_rows.double().mean())
    # decided order: every gap between consecutive float64 scores of the top k+1 admissible columns exceeds the sum of their bars
    r1 = reference(X, Y, k + 1, excluded, j_base)
    real = r1.indices >= 0
    loc = (r1.indices - j_base).clamp(min=0)
    e1 = r.E.gather(1, loc)
    gap = r1.scores[:, :-1] - r1.scores[:, 1:]
    both = real[:, :-1] & real[:, 1:]
    r.decided = (~both | (gap > e1[:, :-1] + e1[:, 1:])).all(1)
    return r


def interval_violations(r, scores, indices):
    """Complaints about a kernel's (or emulation's) [n,k] lists against intervals(); empty = every check holds on EVERY row."""
    bad = []
    n, N = r.s.shape
    k, jb = r.k, r.j_base
    if tuple(scores.shape) != (n, k) or tuple(indices.shape) != (n, k):
        return [f"shapes {tuple(scores.shape)} / {tuple(indices.shape)}, want {(n, k)}"]
    scores, indices = scores.double(), indices.long()
    for i in range(n):
        real = indices[i] >= 0
        m = int(real.sum())
        want = min(k, int(r.n_adm[i]))
        if m != want or not bool(real[:m].all()):
            bad.append(f"row {i}: {m} real entries (or padding in front of one), want {want}")
            continue
        if not (bool((scores[i, m:] == NINF).all()) and bool((indices[i, m:] == -1).all())):
            bad.append(f"row {i}: padding is not -inf / -1")
        loc = indices[i, :m] - jb
        if bool(((loc < 0) | (loc >= N)).any()):
            bad.append(f"row {i}: an index outside the gallery")
            continue
        if len(set(loc.tolist())) != m:
            bad.append(f"row {i}: an index twice")
        if bool(r.excluded[i, loc].any()):
            bad.append(f"row {i}: an excluded column")
        if bool(((scores[i, :m] - r.s[i, loc]).abs() > r.E[i, loc]).any()):
            bad.append(f"row {i}: a score outside the bar of its own index")
        ds = scores[i, 1:m] - scores[i, :m - 1]
        if bool((ds > 0).any()) or bool(((ds == 0) & (loc[1:] <= loc[:-1])).any()):
            bad.append(f"row {i}: not sorted by (score descending, index ascending)")
        have = torch.zeros(N, dtype=torch.bool)
        have[loc] = True
        if bool((r.sure_in[i] & ~have).any()):
            bad.append(f"row {i}: a surely-in column is missing")
        if bool((r.sure_out[i] & have).any()):
            bad.append(f"row {i}: a surely-out column is present")
        if bool(r.decided[i]) and not torch.equal(indices[i], r.indices[i]):
            bad.append(f"row {i}: the order is decided and the indices are not the reference's")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
def exact_case(n_loc, N, D, diag_off, seed=0):
    """Integer rows in {-2..2}.  The gallery is random with every seventh row a copy of the one before it (a planted tie for every
    query); even queries are their diagonal partner plus noise in {-1,0,1} (clamped), so that partner stands near the top, odd
    queries are random."""
    g = torch.Generator().manual_seed(1000 * N + D + seed)
    Y = torch.randint(-2, 3, (N, D), generator=g).float()
    j = torch.arange(N)
    dup = (j % 7 == 3) & (j > 0)
    Y[dup] = Y[j[dup] - 1]
    X = torch.randint(-2, 3, (n_loc, D), generator=g).float()
    partner = (diag_off + torch.arange(n_loc)).clamp(max=N - 1)
    near = (Y[partner] + torch.randint(-1, 2, (n_loc, D), generator=g).float()).clamp(-2, 2)
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


# ---------------------------------------------------------------------------------------------------------------------------------
# emulation of the kernel (fp32 torch) and its mutations
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("ties_high", "pad_col", "pad_row", "no_exclusion", "no_jbase_diag", "no_jbase_index", "kth_dropped", "skip_wave", "skip_half",
             "acc_overwrite")


def _pad_to(t, rows):
    if t.shape[0] == rows:
        return t
    return torch.cat([t, t[-1:].expand(rows - t.shape[0], *t.shape[1:])])


def _select(s, J, k, ties_high=False):
    """The k first of every row's candidates (s fp32 [R,C], J int64 [R,C], J < 0 = not a candidate) under (score descending, J
    ascending), padded with -inf / -1: two stable sorts."""
    R, C = s.shape
    real = J >= 0
    s = torch.where(real, s, torch.full_like(s, NINF))
    J = torch.where(real, J, torch.full_like(J, -1))
    by_j = torch.sort(torch.where(real, -J if ties_high else J, torch.full_like(J, _LAST)), dim=1, stable=True).indices
    s, J = s.gather(1, by_j), J.gather(1, by_j)
    by_s = torch.sort(s, dim=1, descending=True, stable=True).indices
    s, J = s.gather(1, by_s)[:, :k], J.gather(1, by_s)[:, :k]
    if C < k:
        s = torch.cat([s, s.new_full((R, k - C), NINF)], dim=1)
        J = torch.cat([J, J.new_full((R, k - C), -1)], dim=1)
    return s, J


def emulate(X, Y, k, exclude=0, row_key=None, col_label=None, diag_off=0, j_base=0, out=None, mut=None):
    """-> scores fp32 [n,k], indices int32 [n,k], computed on padded tiles; `out` = (scores, indices) already in the buffers."""
    assert mut is None or mut in MUTATIONS, mut
    n, N = X.shape[0], Y.shape[0]
    np_, Np = 32 * math.ceil(n / 32), 32 * math.ceil(N / 32)
    s = _pad_to(X.float(), np_) @ _pad_to(Y.float(), Np).t()
    ig, jg = torch.arange(np_), torch.arange(Np)
    J = (jg if mut == "no_jbase_index" else j_base + jg)[None, :].expand(np_, Np)
    if exclude == 1:
        gone = ((jg if mut == "no_jbase_diag" else j_base + jg)[None, :] == (diag_off + ig)[:, None])
    elif exclude == 2:
        gone = _pad_to(col_label, Np)[None, :] == _pad_to(row_key, np_)[:, None]
    else:
        gone = torch.zeros(np_, Np, dtype=torch.bool)
    if mut == "no_exclusion":
        gone = torch.zeros(np_, Np, dtype=torch.bool)
    if mut != "pad_col":
        gone = gone | (jg >= N)[None, :]
    J = torch.where(gone, torch.full_like(J, -1), J)
    kk = k - 1 if mut == "kth_dropped" else k                    # what a list keeps
    high = mut == "ties_high"
    wave_of, half_of = (jg // 32) % 4, (jg >> 2) & 1
    lists = []
    for w in range(4):
        cols = wave_of == w
        if mut == "skip_half":
            cols = cols & (half_of == 0)
        ls, lj = _select(s[:, cols], J[:, cols], kk, high)
        if w == 0 and out is not None and mut != "acc_overwrite":   # the seed: what the buffers hold (a padded row starts empty)
            os_, oj = out[0].float(), out[1].long()
            fill = np_ - n
            os_ = torch.cat([os_, os_.new_full((fill, k), NINF)])
            oj = torch.cat([oj, oj.new_full((fill, k), -1)])
            ls, lj = _select(torch.cat([os_, ls], dim=1), torch.cat([oj, lj], dim=1), kk, high)
        if mut == "skip_wave" and w == 1:
            continue
        lists.append((ls, lj))
    ms, mj = _select(torch.cat([a for a, _ in lists], dim=1), torch.cat([b for _, b in lists], dim=1), k, high)
    rows = np_ if mut == "pad_row" else n
    return ms[:rows].contiguous(), mj[:rows].int().contiguous()


def emulate_chunked(X, Y, k, exclude, row_key, col_label, diag_off, cuts, mut=None):
    """The gallery streamed as the column chunks `cuts` through j_base / accumulate."""
    out = None
    for a, b in cuts:
        lab = None if col_label is None else col_label[a:b]
        if out is not None:                                      # (the buffers have n rows, whatever a mutation wrote beyond them)
            out = (out[0][:X.shape[0]], out[1][:X.shape[0]])
        out = emulate(X, Y[a:b], k, exclude, row_key, lab, diag_off, a, out, mut)
    return out


class TorchTopKBackend:
    """`head._HipTopKBackend` restated with emulate(): what the CPU / gloo tests install in its place."""
    supported = staticmethod(supported)

    @staticmethod
    def topk(x_loc, y, k, exclude=0, row_key=None, col_label=None, diag_off=0, j_base=0, out=None):
        scores, indices = emulate(x_loc, y, k, exclude, row_key, col_label, diag_off, j_base, out)
        if out is None:
            return scores, indices
        out[0].copy_(scores)
        out[1].copy_(indices)
        return out
