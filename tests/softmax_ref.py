"""Float64 references, exact-data regimes, derived error bars and an fp32 emulation (with mutations) for the softmax contrastive
heads on the tile skeleton csrc/clip_tile.h: the label sources DiagLabel / RowLabel of rows_lse_fwd_kernel and the pair rules
ClipFusedPair, ClipDensePair (csrc/clip_head.hip), LabelledRowPair, LabelledColPair (csrc/averaged_head.hip) of rows_bwd_kernel, and
for the small kernels around them (l2norm, ce_rows, clip_loss_reduce, cluster_mean_cols, cluster_centroids).

Imported by tests/test_softmax_ref_cpu.py (no GPU) and tests/test_softmax_heads_gpu.py (the kernels against the same references).
Everything here runs on the CPU.  The conventions are those of tests/sigmoid_ref.py, whose pieces are imported, not restated.

The operations (X [n,D] local rows, Y [N,D], fp32; s an fp32 scalar; z_ij = s <X_i,Y_j>):
  rows_fwd   lse_i = log sum_j exp z_ij;  pos_i = z_{i,label(i)}, 0 for a label outside [0,N);  optionally logits = z (row pitch ldl)
             label(i) = diag_off + i (DiagLabel) or row_label[i] (RowLabel)
  rows_bwd   dX = [dX0 +] s g Y;  dscale = F + sum_ij g_ij <X_i,Y_j> (F = the pre-fill);  c_up = coef gout;  the lse vectors are INPUTS
     fused   g_ij = c_up (exp(z_ij - lse_row[i]) + exp(z_ij - lse_col[j]) - 2 [j == diag_off + i])
     dense   g_ij = Ga[i,j] + Gb[j,i]                                 (either may be absent; pitches lda, ldb)
     row     g_ij = c_up (exp(z_ij - lse[i]) - [j == label[i]])            lse, label: [n]
     col     g_ij = c_up w_i (exp(z_ij - lse[j]) - [label[j] == key_i])    lse, label: [N];  key_i = row_key ? row_key[i] : key_off + i;
             w_i = counts ? 1 / counts[key_i] : 1;  no dscale
  l2norm     y = x / |x|, norm = |x|;  dx = (dy - y <y,dy>) / norm       (no epsilon: a zero row gives NaN, here as on the device)
  ce_rows    lse_r = log sum_c exp z_rc;  loss = F + weight sum_r (lse_r - z_{r,label(r)}), label(r) = labels ? labels[r] : r;
             dlogits_rc = weight gout (exp(z_rc - lse_r) - [c == label(r)])      (row pitches ld, ldd >= C)
  loss_reduce        loss = F + coef (sum_i (lse_a - pos_a)_i [+ sum_i (lse_b - pos_b)_i])
  cluster_mean_cols  out_ic = mean_{j : labels[j] = c} logits_ij;  dlogits_ij = dout_{i,labels[j]} / counts[labels[j]]
  cluster_centroids  out_c = mean_{j : labels[j] = c} T_j, members added in ascending j; an empty cluster gives a zero row

Bars (u = 2^-24, first order, carried through absolute values; Kd(n) = 2 n + 16 as in sigmoid_ref).  The skeleton's summation tree is
sigmoid_ref's: T = 16 ceil(ceil(N / 32) / 4) + 3 additions at most on any term's path (tree_depth).
  <x,y>   E_dot = Kd(D) u sum_d |x_d||y_d|
  z       E_z = |s| E_dot + 2 u |z|                         (also the bar of the logits and of pos)
  exp     __expf(a) is v_exp_f32(a log2 e): the product is rounded in fp32, an ABSOLUTE error u |a| log2 e in the exponent, so the
          RELATIVE error of the result grows with |a|: K_EXP u (1 + |a|).  Results below the smallest normal are flushed: FLUSH = 2^-126.
  lse     logsumexp is 1-Lipschitz in the sup norm: max_j E_z.  The online merge: column j's term reaches the final sum l through at
          most T + 1 exponentials (its own and one rescale per merge) whose arguments telescope to m - z_j <= |z_j - lse|, and through
          2 T roundings (a product and an addition per merge); with p_j = exp(z_j - lse) the weights of d lse = sum_j p_j d(term_j):
          E_merge = u (K_EXP sum_j p_j (T + 1 + |z_j - lse|) + 2 T).  m + __logf(l): K_LOG u (1 + |log l|) + u |lse|.
          E_lse = max_j E_z + E_merge + K_LOG u (1 + log l) + u |lse|
  p       p = exp(z - lse) with lse an exact fp32 input:  E_p = p (E_z + u |z - lse| + K_EXP u (1 + |z - lse|)) + FLUSH
  g       fused: |c_up| (E_p_row + E_p_col + u (p_row + p_col)) + 3 u |g|     (the sum; c_up's product, the -2, the product with c_up)
          row:   |c_up| E_p + 3 u |g|;   col: |c_up w| E_p + 5 u |g|  (1 / counts and its product more);   dense: u |g| (one addition)
  dX      |s| (E_g |Y| + Kd(N) u |g||Y|) + u |dX - dX0| + [accumulate] u |dX|
  dscale  sum (E_g |dot| + |g| E_dot + u |g dot|) + A u (sum |g dot| + |F|),  A = T + 6 + 3 + blocks + ranks + 1 as in sigmoid_ref
  Row-wise kernels (one wave per row): a lane adds ceil(C / 64) terms, the butterfly 6 more: W(C) = ceil(C / 64) + 6.
  l2norm  norm: sqrt halves the relative error of sum x^2 ((W + 1) u with the squares), and rounds: |x| u ((W + 1) / 2 + 1);
          y: |y| (E_norm / norm + u);  dx: (|y| E_s + u |y s| + u |dy - y s|) / norm + 3 u |dx|, E_s = (W + 1) u sum |y dy|  (s = <y,dy>)
  ce      E_lse = u (sum_c p_c ((K_EXP + 1) |z_c - m| + K_EXP) + W) + K_LOG u (1 + log l) + u |lse|   (logits are exact inputs)
          loss: |weight| sum_r (E_lse + u |lse - z|) + u sum_r |t_r| + (rows + 1) u (sum_r |t_r| + |F|), t_r = weight (lse_r - z): one float
          atomic per row, bounded for ANY order;   dlogits: |g| (E_p at E_z = 0) + 3 u |dlogits|
  reduce  t_i = lse - pos (one rounding each), a thread adds sides ceil(n / 256) of them, butterfly 6, four waves 3, coef, the atomic:
          |coef| (sides ceil(n / 256) + 10) u sum |t| + u (|coef sum t| + |loss| + |F|)
  mean    LDS float atomics in any order: a sum of c numbers carries at most (c - 1) u sum |.|, the division u more;  bwd: u |dlogits|
K_EXP and K_LOG, the accuracy of the device's __expf / __logf, are measured, not derived (see below).

Exact regimes.  integer_case: X, Y, Ga, Gb small integers, s = 4: every product and every fp32 partial sum is an integer below 2^24,
so logits, pos, dX and dscale are exact; the operands are not symmetric (Ga != Gb^T, n != N in most shapes).  onehot_case: one-hot
rows, s = 256, z in {0, 256}, every lse input 256: exp(0) = 1 and exp(-256) = 2^-369 rounds (flushes) to 0, so g = c_up x a small
integer; coef, gout, 1 / counts powers of two.  Forward: a row with exactly ONE matching column has l = 1, lse = 256 + log 1 = 256,
pos in {0, 256}; other rows belong to the Gaussian regime only.  exactness_violations() asserts all this on the reference alone and
rejects a vacuous case (every g zero, or no exact forward row).

The emulation (emulate) is the kernels' arithmetic in fp32 torch on tiles padded as clip_tile.h pads them (rows >= n_loc and columns
>= N are clamped duplicates of the last valid one, then selected to zero), the forward with the per-(wave, half, tile) online
softmax and the merges in the kernel's order.  MUTATIONS break one thing at a time; mutation_applies says where one is visible."""
import math
import types

import torch

from tests.sigmoid_ref import COLS_PER_PASS, Kd, U, _pad_to, f32, gaussian_case, hand_labels, ratio  # noqa: F401  (re-exported)
from tests import sigmoid_ref as _S

# Accuracy of the device's __expf / __logf, in units of u (1 + |argument|) and u (1 + |log l|).  Measured against the float64
# reference with both at 1 on the MI355X by tests/test_softmax_heads_gpu.py (the rows with "k_exp": 1.0 of
# profiles/softmax_measured_tolerances.jsonl); the rule is sigmoid_ref's (above K_FN): the smallest power of two that is at least 4
# times the worst ratio measured at 1.
# K_EXP: of the outputs whose bar holds K_EXP the worst was 0.8888, dlogits of mmg_ce_rows_bwd at C = 200 (row "softmax_ce_rows",
#        "C": 200) - a bar that is the exponential's alone, the logits and lse being exact inputs; 4 x 0.8888 = 3.56 gives 4.  On the
#        skeleton, where E_z (the fp32 dot product) dominates, the worst was 0.516 (col.dX at (8, 5, 32, 0)).
# K_LOG: only lse (and the loss summed from it) holds it; the worst was 0.6035, lse of mmg_ce_rows_fwd at C = 200 (the same rows);
#        4 x 0.6035 = 2.41 gives 4.  The skeleton's lse stayed below 0.016.
# The rows with "k_exp": 4.0 are the ratios under the constants as set.
K_EXP = 4.0
K_LOG = 4.0
FLUSH = 2.0 ** -126
NEG_BIG = -1.0e30            # clip_tile.h

# (n_loc, N, D, diag_off).  sigmoid_ref.SHAPES (one pair; a partial tile; a tile and one more; three row tiles at the widest D, NDT = 8;
# one column more than a workgroup pass, NDT = 4; a rank that is not the first; two NDT = 2 shapes) and:
#   (33, 33, 96, 0)   D / 32 = 3: NDT = 1 and wave 3 owns no d tile in the second product
#   (34, 35, 160, 0)  D / 32 = 5: NDT = 2 and waves 1..3 own no second d tile
#   (40, 5, 64, 0)    rectangular zero-shot: N < 32, N % 4 != 0, rows 5.. have a diagonal label outside [0, N); two row blocks
#   (8, 5, 32, 0)     rows 5..7 have a label outside [0, N)
# WRITE_LOGITS' float4 store runs where j + 3 < N and ldl % 4 == 0, the scalar tail otherwise: every N here that is no multiple of 4
# takes both at ldl = N rounded up to 4, and only the tail at ldl = N + 1.
SHAPES = _S.SHAPES + ((33, 33, 96, 0), (34, 35, 160, 0), (40, 5, 64, 0), (8, 5, 32, 0))
SCALES = (14.2857, 100.0)
OPS = ("fwd_diag", "fwd_label", "fused", "dense", "row", "col")
EXACT_S, EXACT_LSE, INT_S = 256.0, 256.0, 4.0


def ndt_of(D):
    """The NDT instantiation launch_rows_bwd takes."""
    n = (D + 127) // 128
    return 1 if n <= 1 else 2 if n == 2 else 4 if n <= 4 else 8


def kernel_note(op, D=None, logits=False):
    """mmg_last_kernel() after the launch of `op`."""
    if op in ("fwd_diag", "fwd_label"):
        return "rows_lse_fwd_kernel<%s, %s>" % ("DiagLabel" if op == "fwd_diag" else "RowLabel", "true" if logits else "false")
    pair = {"fused": "ClipFusedPair", "dense": "ClipDensePair", "row": "LabelledRowPair", "col": "LabelledColPair"}[op]
    return "rows_bwd_kernel<%s, %d>" % (pair, ndt_of(D))


def tree_depth(N):
    return 16 * math.ceil(math.ceil(N / 32) / 4) + 3


def atomics(n, N, ranks=1):
    return tree_depth(N) + 6 + 3 + math.ceil(n / 32) + ranks + 1


def W(C):
    return math.ceil(C / 64) + 6


# ---------------------------------------------------------------------------------------------------------------------------------
# cases: one launch of one entry point, its operands as CPU tensors / Python numbers
# ---------------------------------------------------------------------------------------------------------------------------------
def _case(op, X, Y, s, **kw):
    c = types.SimpleNamespace(op=op, X=X.contiguous(), Y=Y.contiguous(), s=f32(s), n=X.shape[0], N=Y.shape[0], D=X.shape[1], diag_off=0,
                              row_label=None, ldl=None, lse_row=None, lse_col=None, gout=None, coef=1.0, dscale0=None, Ga=None, Gb=None,
                              lda=None, ldb=None, accumulate=0, dX0=None, col_label=None, row_key=None, key_off=0, counts=None, ranks=1)
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return c


def row_labels(n, N):
    """RowLabel's labels, made by hand: a stride through the columns, row 0 its own index's neighbour, and - as soon as there are five
    rows - labels outside [0, N) on both sides (N + 2 at i % 5 == 4, -1 at i % 11 == 7)."""
    i = torch.arange(n)
    lab = (7 * i + 3) % N
    lab = torch.where(i % 5 == 4, torch.full_like(lab, N + 2), lab)
    return torch.where(i % 11 == 7, torch.full_like(lab, -1), lab).to(torch.int64)


def labels_of(case):
    """The label of every local row of a forward / row case (int64 [n])."""
    return case.diag_off + torch.arange(case.n) if case.row_label is None else case.row_label


def seed_for(shape):
    """Seeds of the Gaussian cases.  (32, 129, 512, 0) is the one shape with more than four column tiles: its seed is one at which the
    reference shows a row whose maximum is not in the first tile its lane meets (mutation_applies(.., "no_rescale") asserts it)."""
    return 7 * shape[1] + shape[2] + (1 if tuple(shape) == (32, COLS_PER_PASS + 1, 512, 0) else 0)


def gaussian_cases(shape, scale):
    """name -> case: every entry point and variant the Gaussian regime runs at one shape and scale."""
    n, N, D, off = shape
    X, Y = gaussian_case(n, N, D, seed_for(shape))
    s = f32(scale)
    z = s * (X.double() @ Y.double().t())
    lse_row = torch.logsumexp(z, 1).float()
    lse_col = (torch.logsumexp(z, 0) + math.log(max(N / n, 1.0))).float()       # what the other ranks' rows would add, roughly
    coef = f32(1.0 / (2 * N))
    rl = row_labels(n, N)
    g = torch.Generator().manual_seed(seed_for(shape) + 1)
    ld4 = 4 * math.ceil(N / 4)
    lda, ldb = N + 3, n + 5
    Ga = (torch.randn(n, lda, generator=g) / N).contiguous()
    Gb = (torch.randn(N, ldb, generator=g) / N).contiguous()
    dX0 = torch.randn(n, D, generator=g).contiguous()
    cl = hand_labels(N)
    key = cl[(off + torch.arange(n)).clamp(max=N - 1)].clone()
    counts = torch.bincount(cl, minlength=N).to(torch.int32)
    out = {"fwd": _case("fwd_diag", X, Y, s, diag_off=off),
           "fwd_logits_ldN": _case("fwd_diag", X, Y, s, diag_off=off, ldl=N),
           "fwd_logits_ld4": _case("fwd_diag", X, Y, s, diag_off=off, ldl=ld4),
           "fwd_logits_ldN1": _case("fwd_diag", X, Y, s, diag_off=off, ldl=N + 1),
           "fwd_label": _case("fwd_label", X, Y, s, row_label=rl),
           "fused": _case("fused", X, Y, s, diag_off=off, lse_row=lse_row, lse_col=lse_col, coef=coef, gout=None, dscale0=0.5),
           "fused_gout": _case("fused", X, Y, s, diag_off=off, lse_row=lse_row, lse_col=lse_col, coef=coef, gout=0.25, dscale0=0.5),
           "fused_nods": _case("fused", X, Y, s, diag_off=off, lse_row=lse_row, lse_col=lse_col, coef=coef, gout=0.25),
           "dense_a": _case("dense", X, Y, s, Ga=Ga, lda=lda, dscale0=0.5),
           "dense_b": _case("dense", X, Y, s, Gb=Gb, ldb=ldb, dscale0=0.5),
           "dense_ab": _case("dense", X, Y, s, Ga=Ga, lda=lda, Gb=Gb, ldb=ldb, dscale0=0.5),
           "row": _case("row", X, Y, s, lse_row=lse_row, row_label=rl, coef=coef, gout=0.25, dscale0=0.5),
           "row_acc": _case("row", X, Y, s, lse_row=lse_row, row_label=rl, coef=coef, gout=None, dscale0=0.5, accumulate=1, dX0=dX0),
           "col_off": _case("col", X, Y, s, lse_col=lse_col, col_label=cl, key_off=off, coef=coef, gout=0.25),
           "col_key": _case("col", X, Y, s, lse_col=lse_col, col_label=cl, row_key=key, counts=counts, coef=coef, gout=None, accumulate=1,
                            dX0=dX0)}
    return out


def dense_scale_cases(shape):
    """The dense rule at s = 1 (its scale in the similarity product of the clustering)."""
    return {k: v for k, v in gaussian_cases(shape, 1.0).items() if k.startswith("dense")}


def integer_case(shape, op, **kw):
    """Small-integer operands, s = 4.  X has eight non-zero columns per row (one of them the last, for row 0), so |<X_i,Y_j>| <= 32 and the
    accumulated scalar stays far below 2^24 quanta; Y is dense in every column, so every d tile of dX is exercised."""
    n, N, D, off = shape
    i, j, d = torch.arange(n)[:, None], torch.arange(N)[:, None], torch.arange(D)[None, :]
    X = torch.zeros(n, D)
    for k in range(8):
        X[torch.arange(n), ((k * (D - 1)) // 7 + torch.arange(n)) % D] = ((torch.arange(n) + 2 * k) % 5 - 2).float()
    Y = ((3 * j + d) % 5 - 2).float()
    lda, ldb = N + 3, n + 5
    Ga = torch.full((n, lda), 99.0)
    Ga[:, :N] = ((2 * i + 3 * torch.arange(N)[None, :]) % 5 - 2).float()
    Gb = torch.full((N, ldb), -99.0)
    Gb[:, :n] = ((3 * torch.arange(n)[None, :] + j) % 4 - 1).float()
    if op == "fwd_diag":
        return _case(op, X, Y, INT_S, diag_off=off, **kw)
    return _case("dense", X, Y, INT_S, **{**dict(Ga=Ga, lda=lda, Gb=Gb, ldb=ldb, dscale0=0.5), **kw})


def onehot_case(shape, op, **kw):
    """One-hot rows, s = 256.  Backward (fused / row / col): sigmoid_ref.exact_case's rows - four directions, every fifth column shifted
    by one - so a row matches about N / 4 columns and its label column is often not among them; every lse input is 256.
    Forward: X_i = e_{a_i}, a_i = (gi + [gi % 3 == 1]) % D; Y_j = e_{j % D} for the D - 1 columns from diag_off on and one spare
    direction for every other column: row i matches exactly one column (if that column exists), its label's only where gi % 3 != 1."""
    n, N, D, off = shape
    gi = off + torch.arange(n)
    if op in ("fwd_diag", "fwd_label"):
        a = (gi + (gi % 3 == 1).long()) % D
        j = torch.arange(N)
        cdir = torch.where((j >= off) & (j < off + D - 1), j % D, torch.full_like(j, (off + D - 1) % D))
        X, Y = torch.zeros(n, D), torch.zeros(N, D)
        X[torch.arange(n), a] = 1.0
        Y[j, cdir] = 1.0
        if op == "fwd_diag":
            return _case(op, X, Y, EXACT_S, diag_off=off, **kw)
        return _case(op, X, Y, EXACT_S, row_label=torch.where(torch.arange(n) % 5 == 4, torch.full_like(gi, N + 2), gi), **kw)
    X, Y, _, _ = _S.exact_case(n, N, D, off, False)
    coef = 2.0 ** -math.ceil(math.log2(2 * N))
    lse_n, lse_N = torch.full((n,), EXACT_LSE), torch.full((N,), EXACT_LSE)
    dX0 = (((torch.arange(n)[:, None] + torch.arange(D)[None, :]) % 7 - 3) * (EXACT_S * coef)).float()
    base = dict(coef=coef, dX0=dX0)
    if op == "fused":
        base.update(diag_off=off, lse_row=lse_n, lse_col=lse_N, dscale0=0.5, dX0=None)
    elif op == "row":
        base.update(lse_row=lse_n, row_label=row_labels(n, N), dscale0=0.5)
    else:
        assert op == "col", op
        cl = hand_labels(N)
        base.update(lse_col=lse_N, col_label=cl)
        if kw.pop("keyed", False):                  # 1 / counts is a power of two: counts 1, 2, 4
            base.update(row_key=cl[gi.clamp(max=N - 1)].clone(), counts=(2 ** (torch.arange(N) % 3)).to(torch.int32))
        else:
            base.update(key_off=off)
    return _case(op, X, Y, EXACT_S, **{**base, **kw})


def exact_cases(shape):
    """name -> case: every entry point and variant of the exact regimes at one shape."""
    N = shape[1]
    return {"int_logits_ldN": integer_case(shape, "fwd_diag", ldl=N),
            "int_logits_ld4": integer_case(shape, "fwd_diag", ldl=4 * math.ceil(N / 4)),
            "int_logits_ldN1": integer_case(shape, "fwd_diag", ldl=N + 1),
            "int_dense_a": integer_case(shape, "dense", Gb=None, ldb=None),
            "int_dense_b": integer_case(shape, "dense", Ga=None, lda=None),
            "int_dense_ab": integer_case(shape, "dense"),
            "int_dense_ab_nods": integer_case(shape, "dense", dscale0=None),
            "hot_fwd": onehot_case(shape, "fwd_diag"),
            "hot_fwd_label": onehot_case(shape, "fwd_label"),
            "hot_fused": onehot_case(shape, "fused"),
            "hot_fused_gout": onehot_case(shape, "fused", gout=0.25),
            "hot_fused_nods": onehot_case(shape, "fused", gout=0.25, dscale0=None),
            "hot_row": onehot_case(shape, "row", gout=0.25),
            "hot_row_acc": onehot_case(shape, "row", accumulate=1),
            "hot_col_off": onehot_case(shape, "col", gout=0.25),
            "hot_col_off_acc": onehot_case(shape, "col", accumulate=1),
            "hot_col_key": onehot_case(shape, "col", keyed=True, accumulate=1)}


def exact_mismatches(c, ref, got):
    """Names of the outputs that are not bit for bit the reference's (rounded to fp32, which is exact for them).  One-hot forward: the
    rows with exactly one matching column; integer forward: logits and pos (its lse belongs to the Gaussian regime)."""
    bad = []
    fwd = c.op in ("fwd_diag", "fwd_label")
    rows = exact_rows(c) if fwd and c.s == EXACT_S else slice(None)
    for name, (want, _) in ref.items():
        if fwd and c.s == INT_S and name == "lse":
            continue
        g = torch.as_tensor(got[name]).float().reshape(want.shape)
        if not torch.equal(g[rows] if fwd else g, (want[rows] if fwd else want).float()):
            bad.append(name)
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference with bars
# ---------------------------------------------------------------------------------------------------------------------------------
def _E_p(p, a, E_z, k_exp):
    """Bar of p = exp(a), a = z - lse computed in fp32 from an exact lse."""
    return p * (E_z + U * a.abs() + k_exp * U * (1 + a.abs())) + FLUSH


def pair_weights(c, z, dot, E_z, k_exp):
    """g [n,N] of a backward case and its bar, float64."""
    n, N = c.n, c.N
    i, j = torch.arange(n)[:, None], torch.arange(N)[None, :]
    if c.op == "dense":
        g = torch.zeros(n, N, dtype=torch.float64)
        if c.Ga is not None:
            g = g + c.Ga[:, :N].double()
        if c.Gb is not None:
            g = g + c.Gb[:, :n].double().t()
        return g, U * g.abs() * (c.Ga is not None and c.Gb is not None)
    c_up = float(f32(c.coef)) * (1.0 if c.gout is None else float(f32(c.gout)))
    if c.op == "fused":
        ar, ac = z - c.lse_row.double()[:, None], z - c.lse_col.double()[None, :]
        pr, pc = torch.exp(ar), torch.exp(ac)
        g = c_up * (pr + pc - 2.0 * (j == c.diag_off + i))
        return g, abs(c_up) * (_E_p(pr, ar, E_z, k_exp) + _E_p(pc, ac, E_z, k_exp) + U * (pr + pc)) + 3 * U * g.abs()
    if c.op == "row":
        a = z - c.lse_row.double()[:, None]
        p = torch.exp(a)
        g = c_up * (p - 1.0 * (j == c.row_label[:, None]))
        return g, abs(c_up) * _E_p(p, a, E_z, k_exp) + 3 * U * g.abs()
    assert c.op == "col", c.op
    key = (c.key_off + torch.arange(n)) if c.row_key is None else c.row_key
    w = torch.ones(n, dtype=torch.float64)
    if c.counts is not None:
        ok = (key >= 0) & (key < c.counts.shape[0])
        w = torch.where(ok, 1.0 / c.counts[key.clamp(0, c.counts.shape[0] - 1)].double(), w)
    a = z - c.lse_col.double()[None, :]
    p = torch.exp(a)
    g = c_up * w[:, None] * (p - 1.0 * (c.col_label[None, :] == key[:, None]))
    return g, abs(c_up) * w[:, None] * _E_p(p, a, E_z, k_exp) + 5 * U * g.abs()


def reference(c, k_exp=None, k_log=None):
    """name -> (float64 value, bar) of every output of the case's launch."""
    k_exp = K_EXP if k_exp is None else k_exp
    k_log = K_LOG if k_log is None else k_log
    Xd, Yd = c.X.double(), c.Y.double()
    dot, adot = Xd @ Yd.t(), Xd.abs() @ Yd.abs().t()
    z = c.s * dot
    E_dot = Kd(c.D) * U * adot
    E_z = abs(c.s) * E_dot + 2 * U * z.abs()
    T = tree_depth(c.N)
    out = {}
    if c.op in ("fwd_diag", "fwd_label"):
        lse = torch.logsumexp(z, 1)
        lab = labels_of(c)
        inside = (lab >= 0) & (lab < c.N)
        labc = lab.clamp(0, c.N - 1)
        idx = torch.arange(c.n)
        p = torch.exp(z - lse[:, None])
        logl = lse - z.max(1).values
        E_merge = U * (k_exp * (p * (T + 1 + (z - lse[:, None]).abs())).sum(1) + 2 * T)
        out["lse"] = (lse, E_z.max(1).values + E_merge + k_log * U * (1 + logl) + U * lse.abs())
        out["pos"] = (torch.where(inside, z[idx, labc], torch.zeros_like(lse)), torch.where(inside, E_z[idx, labc], torch.zeros_like(lse)))
        if c.ldl is not None:
            out["logits"] = (z, E_z)
        return out
    g, E_g = pair_weights(c, z, dot, E_z, k_exp)
    dX = c.s * (g @ Yd)
    E_dX = abs(c.s) * (E_g @ Yd.abs() + Kd(c.N) * U * (g.abs() @ Yd.abs())) + U * dX.abs()
    if c.accumulate:
        dX = dX + c.dX0.double()
        E_dX = E_dX + U * dX.abs()
    out["dX"] = (dX, E_dX)
    if c.dscale0 is not None and c.op != "col":
        gd = (g * dot).abs()
        out["dscale"] = (c.dscale0 + (g * dot).sum(),
                         (E_g * dot.abs() + g.abs() * E_dot + U * gd).sum() + atomics(c.n, c.N, c.ranks) * U * (gd.sum() + abs(c.dscale0)))
    return out


def ratios(ref, got):
    """name -> ratio of every output of `ref`; `got` must hold them all."""
    return {k: ratio(got[k], v, E) for k, (v, E) in ref.items()}


def exact_rows(c):
    """Rows of a one-hot forward case with exactly one matching column (bool [n])."""
    return ((c.X.double() @ c.Y.double().t()) == 1.0).sum(1) == 1


def exactness_violations(c, ref):
    """Preconditions of the exact regimes, on the case and its float64 reference alone.  Returns a list of complaints (empty = a
    torch.equal comparison is justified and not vacuous)."""
    bad = []
    dot = c.X.double() @ c.Y.double().t()
    two24 = 2.0 ** 24

    def dyadic(name, v, q):
        k = torch.as_tensor(v).double() / q
        if not bool(((k - k.round()).abs() * q < 1e-50).all()) or float(k.abs().max()) >= two24:     # (float64 keeps exp(-256) = 1e-111)
            bad.append(f"{name} is not a sum of fewer than 2^24 quanta of {q}")
    if c.s == INT_S:                                   # integer regime
        for name, t in (("X", c.X), ("Y", c.Y)) + ((("Ga", c.Ga[:, :c.N]),) if c.Ga is not None else ()) + ((("Gb", c.Gb[:, :c.n]),) if c.Gb is not None else ()):
            if not bool((t == t.round()).all()):
                bad.append(f"{name} is not integer")
        if float((c.X.abs().double() @ c.Y.abs().double().t()).max()) * INT_S >= two24:
            bad.append("a dot product's partial sums may leave 2^24")
        if c.op == "dense":
            g, _ = pair_weights(c, c.s * dot, dot, torch.zeros_like(dot), 0.0)
            if not bool((g != 0).any()) or bool((g == g.t()).all() if c.n == c.N > 1 else False):
                bad.append("vacuous: g is zero or symmetric")
            if c.Ga is not None and c.Gb is not None and c.n == c.N and torch.equal(c.Ga[:, :c.N], c.Gb[:, :c.n]):
                bad.append("vacuous: Ga equals Gb, a transposed read cannot show")
            if float(INT_S * (g.abs() @ c.Y.abs().double()).max()) >= two24:
                bad.append("dX's partial sums may leave 2^24")
            if c.dscale0 is not None and ((g * dot).abs().sum() + abs(c.dscale0)) / 0.5 >= two24:
                bad.append("dscale's partial sums may leave 2^24 quanta")
        return bad
    if c.s != EXACT_S:
        return ["not an exact case"]
    if not bool(((dot == 0) | (dot == 1)).all()):
        bad.append("<X_i,Y_j> is not 0 or 1")
    if c.op in ("fwd_diag", "fwd_label"):
        rows = exact_rows(c)
        if not bool(rows.any()):
            bad.append("vacuous: no row with exactly one matching column")
        else:
            lse, pos = ref["lse"][0][rows], ref["pos"][0][rows]
            if not bool(((lse - EXACT_S).abs() < 1e-50).all()):
                bad.append("an exact row's lse is not 256")
            if not bool(((pos == 0) | (pos == EXACT_S)).all()):
                bad.append("an exact row's pos is not 0 or 256")
            if int(rows.sum()) > 2 and c.N > 2 and not (bool((pos == 0).any()) and bool((pos == EXACT_S).any())):
                bad.append("vacuous: the exact rows do not show both pos = 0 and pos = 256")
        return bad
    for name in ("lse_row", "lse_col"):
        v = getattr(c, name)
        if v is not None and not bool((v == EXACT_LSE).all()):
            bad.append(f"{name} is not 256")
    c_up = c.coef * (1.0 if c.gout is None else c.gout)
    if math.frexp(c_up)[0] != 0.5:
        bad.append("coef * gout is not a power of two")
    if c.counts is not None and not bool(((c.counts & (c.counts - 1)) == 0).all()):
        bad.append("a count is not a power of two")
    q = abs(c_up) / (4.0 if c.counts is not None else 1.0)
    g, _ = pair_weights(c, c.s * dot, dot, torch.zeros_like(dot), 0.0)
    if not bool((g.abs() > 1e-50).any()):
        bad.append("vacuous: every g is zero (each row's label column is its only matching column)")
    dyadic("g", g, q)
    dyadic("dX", ref["dX"][0], q * EXACT_S)
    if c.accumulate:
        dyadic("dX0", c.dX0, q * EXACT_S)
    if "dscale" in ref:
        qs = min(q, 0.5)
        dyadic("dscale", ref["dscale"][0], qs)
        if ((g * dot).abs().sum() + abs(c.dscale0)) / qs >= two24:
            bad.append("dscale's partial sums may leave 2^24 quanta")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# emulation of the kernels (fp32 torch) and its mutations
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("no_diag_off", "label_vs_index", "pad_col", "pad_row", "no_rescale", "minus_one_not_two", "lse_col_by_row", "gb_untransposed",
             "accumulate_ignored", "counts_ignored", "key_off_ignored", "pos_outside_nonzero", "dscale_overwritten")
_HALF_COLS = tuple(torch.tensor([(r & 3) + 8 * (r >> 2) + 4 * h for r in range(16)]) for h in (0, 1))     # acc_row(r, h)


def _merge(m, l, m2, l2):
    mn = torch.maximum(m, m2)
    return mn, l * torch.exp(m - mn) + l2 * torch.exp(m2 - mn)


def _emulate_fwd(c, mut):
    n, N = c.n, c.N
    np_, Np = 32 * math.ceil(n / 32), 32 * math.ceil(N / 32)
    Xp, Yp = _pad_to(c.X.float(), np_), _pad_to(c.Y.float(), Np)
    s32 = torch.tensor(c.s, dtype=torch.float32)
    z = (Xp @ Yp.t()) * s32
    ig = torch.arange(np_)
    if c.op == "fwd_diag":
        lab = (0 if mut == "no_diag_off" else c.diag_off) + ig
    else:
        lab = ig.clone() if mut == "label_vs_index" else _pad_to(c.row_label, np_)
    if mut == "pos_outside_nonzero":
        lab = lab.clamp(0, N - 1)
    jg = torch.arange(Np)
    valid = torch.ones(Np, dtype=torch.bool) if mut == "pad_col" else jg < N
    neg = torch.full((np_,), NEG_BIG)
    waves = []
    pos = torch.zeros(np_)
    for w in range(4):
        halves = []
        for h in (0, 1):
            m, l = neg.clone(), torch.zeros(np_)
            for jt in range(w, Np // 32, 4):
                cols = 32 * jt + _HALF_COLS[h]
                v = valid[cols]
                zt = z[:, cols]
                hit = (cols[None, :] == lab[:, None]) & v[None, :]
                pos = torch.where(hit.any(1), (zt * hit).sum(1), pos)
                tmax = torch.where(v[None, :], zt, neg[:, None]).max(1).values
                mn = torch.maximum(m, tmax)
                e = torch.where(v[None, :], torch.exp(zt - mn[:, None]), torch.zeros_like(zt))
                ssum = torch.zeros(np_)
                for r in range(16):
                    ssum = ssum + e[:, r]
                l = (l if mut == "no_rescale" else l * torch.exp(m - mn)) + ssum
                m = mn
            halves.append((m, l))
        waves.append(_merge(*halves[0], *halves[1]))
    mm, ll = neg.clone(), torch.zeros(np_)
    for m, l in waves:
        mm, ll = _merge(mm, ll, m, l)
    out = {"lse": (mm + torch.log(ll))[:n], "pos": pos[:n]}
    if c.ldl is not None:
        out["logits"] = z[:n, :N]
    return out


def _emulate_bwd(c, mut):
    n, N = c.n, c.N
    np_, Np = 32 * math.ceil(n / 32), 32 * math.ceil(N / 32)
    Xp, Yp = _pad_to(c.X.float(), np_), _pad_to(c.Y.float(), Np)
    s32 = torch.tensor(c.s, dtype=torch.float32)
    dot = Xp @ Yp.t()
    z = dot * s32
    ig, jg = torch.arange(np_), torch.arange(Np)
    igc, jgc = ig.clamp(max=n - 1), jg.clamp(max=N - 1)
    one = torch.ones((), dtype=torch.float32)
    if c.op == "dense":
        g = torch.zeros(np_, Np)
        if c.Ga is not None:
            g = g + c.Ga[igc][:, jgc]
        if c.Gb is not None:
            if mut == "gb_untransposed":                 # Gb[i * ldb + j]
                flat = c.Gb.reshape(-1)
                g = g + flat[(igc[:, None] * c.ldb + jgc[None, :]).clamp(max=flat.numel() - 1)]
            else:
                g = g + c.Gb[jgc][:, igc].t()
    else:
        c_up = torch.tensor(c.coef, dtype=torch.float32) * (one if c.gout is None else torch.tensor(c.gout, dtype=torch.float32))
        if c.op == "fused":
            lr = _pad_to(c.lse_row, np_)
            lc = c.lse_col[igc.clamp(max=N - 1)][:, None] if mut == "lse_col_by_row" else _pad_to(c.lse_col, Np)[None, :]
            g = torch.exp(z - lr[:, None]) + torch.exp(z - lc)
            diag = jg[None, :] == ((0 if mut == "no_diag_off" else c.diag_off) + ig)[:, None]
            g = (g - (1.0 if mut == "minus_one_not_two" else 2.0) * diag) * c_up
        elif c.op == "row":
            lab = ig.clone() if mut == "label_vs_index" else _pad_to(c.row_label, np_)
            g = (torch.exp(z - _pad_to(c.lse_row, np_)[:, None]) - 1.0 * (jg[None, :] == lab[:, None])) * c_up
        else:
            key = ((0 if mut in ("key_off_ignored", "no_diag_off") else c.key_off) + igc) if c.row_key is None else _pad_to(c.row_key, np_)
            cu = c_up.expand(np_).clone()
            if c.counts is not None and mut != "counts_ignored":
                ok = (key >= 0) & (key < c.counts.shape[0])
                cnt = torch.where(ok, c.counts[key.clamp(0, c.counts.shape[0] - 1)], torch.ones_like(c.counts[:1])).float()
                cu = cu * (one / cnt)
            g = (torch.exp(z - _pad_to(c.lse_col, Np)[None, :]) - 1.0 * (_pad_to(c.col_label, Np)[None, :] == key[:, None])) * cu[:, None]
    valid = torch.ones(np_, Np, dtype=torch.bool)
    if mut != "pad_col":
        valid &= (jg < N)[None, :]
    if mut != "pad_row":
        valid &= (ig < n)[:, None]
    g = torch.where(valid, g, torch.zeros_like(g))
    dX = ((g @ Yp) * s32)[:n]
    if c.accumulate and mut != "accumulate_ignored":
        dX = c.dX0 + dX
    out = {"dX": dX}
    if c.dscale0 is not None and c.op != "col":
        out["dscale"] = (0.0 if mut == "dscale_overwritten" else torch.tensor(c.dscale0, dtype=torch.float32)) + (g * dot).sum()
    return out


def emulate(c, mut=None):
    """name -> fp32 tensor of every output of the case's launch, computed on padded tiles."""
    assert mut is None or mut in MUTATIONS, mut
    return _emulate_fwd(c, mut) if c.op in ("fwd_diag", "fwd_label") else _emulate_bwd(c, mut)


def mutation_applies(c, mut):
    """Is the mutated feature in the case at all?  (Decided on the case and the float64 reference, never on the emulation.)"""
    fwd = c.op in ("fwd_diag", "fwd_label")
    lab = labels_of(c) if fwd or c.op == "row" else None
    if mut == "no_diag_off":
        return c.diag_off != 0 and c.op in ("fwd_diag", "fused")
    if mut == "label_vs_index":
        inside = lambda v: torch.where((v >= 0) & (v < c.N), v, torch.full_like(v, -1))
        return c.op in ("fwd_label", "row") and bool((inside(lab) != inside(torch.arange(c.n))).any())
    if mut == "pad_col":                                    # (one column: its softmax is 1 and every softmax rule's g is 0)
        return c.N % 32 != 0 and (fwd or c.N > 1)
    if mut == "pad_row":                                    # the padded rows repeat the last row: its share of dscale, times their number
        if fwd or c.n % 32 == 0 or c.dscale0 is None or c.op == "col" or c.N == 1:
            return False
        dot = c.X.double() @ c.Y.double().t()
        g, _ = pair_weights(c, c.s * dot, dot, torch.zeros_like(dot), 0.0)
        return (32 - c.n % 32) * abs(float((g * dot)[-1].sum())) > 2 * float(reference(c)["dscale"][1])
    if mut == "no_rescale":
        if not fwd or c.N <= COLS_PER_PASS:
            return False
        z = c.s * (c.X.double() @ c.Y.double().t())
        for w in range(4):                                  # a lane's tiles: jt = w, w + 4, ..; its columns: those of its half
            for h in (0, 1):
                first = 32 * w + _HALF_COLS[h]
                later = torch.cat([32 * jt + _HALF_COLS[h] for jt in range(w + 4, math.ceil(c.N / 32), 4)] or [torch.zeros(0, dtype=torch.long)])
                first, later = first[first < c.N], later[later < c.N]
                if len(first) and len(later) and bool((z[:, later].max(1).values > z[:, first].max(1).values + 0.1).any()):
                    return True
        return False
    if mut == "minus_one_not_two":
        return c.op == "fused" and c.diag_off < c.N
    if mut == "lse_col_by_row":
        return c.op == "fused" and c.N > 1
    if mut == "gb_untransposed":
        return c.op == "dense" and c.Gb is not None and c.N > 1
    if mut == "accumulate_ignored":
        return bool(c.accumulate)
    if mut == "counts_ignored":
        return c.op == "col" and c.counts is not None and bool((c.counts[c.row_key] > 1).any())
    if mut == "key_off_ignored":
        return c.op == "col" and c.row_key is None and c.key_off != 0
    if mut == "pos_outside_nonzero":
        return fwd and bool(((lab < 0) | (lab >= c.N)).any())
    if mut == "dscale_overwritten":
        return (not fwd) and c.op != "col" and c.dscale0 not in (None, 0.0)
    raise AssertionError(mut)


# ---------------------------------------------------------------------------------------------------------------------------------
# the small kernels: float64 value and bar
# ---------------------------------------------------------------------------------------------------------------------------------
def l2norm_fwd(x):
    """-> {y, norm}.  A zero row gives norm 0 and y = 0 / 0 = NaN, here as on the device."""
    xd = x.double()
    D = x.shape[1]
    norm = xd.norm(dim=1)
    y = xd / norm[:, None]
    E_norm = norm * U * ((W(D) + 1) / 2 + 1)
    return {"norm": (norm, E_norm), "y": (y, y.abs() * (E_norm / norm + U)[:, None])}


def l2norm_bwd(y, norm, dy):
    """y, norm, dy are the kernel's fp32 inputs."""
    yd, nd, gd = y.double(), norm.double()[:, None], dy.double()
    D = y.shape[1]
    s = (yd * gd).sum(1, keepdim=True)
    E_s = (W(D) + 1) * U * (yd * gd).abs().sum(1, keepdim=True)
    dx = (gd - yd * s) / nd
    return {"dx": (dx, (yd.abs() * E_s + U * (yd * s).abs() + U * (gd - yd * s).abs()) / nd.abs() + 3 * U * dx.abs())}


def ce_rows_fwd(logits, labels, weight, loss0, k_exp=None, k_log=None):
    """logits [rows, C] (the valid columns), labels int64 [rows] or None (= the row's index) -> {lse, loss}."""
    k_exp = K_EXP if k_exp is None else k_exp
    k_log = K_LOG if k_log is None else k_log
    z = logits.double()
    rows, C = z.shape
    lab = torch.arange(rows) if labels is None else labels
    m = z.max(1, keepdim=True).values
    lse = torch.logsumexp(z, 1)
    p = torch.exp(z - lse[:, None])
    E_lse = U * ((p * ((k_exp + 1) * (z - m).abs() + k_exp)).sum(1) + W(C)) + k_log * U * (1 + (lse - m[:, 0])) + U * lse.abs()
    w = float(f32(weight))
    d = lse - z[torch.arange(rows), lab]
    t = w * d
    loss = loss0 + t.sum()
    E_loss = abs(w) * (E_lse + U * d.abs()).sum() + U * t.abs().sum() + (rows + 1) * U * (t.abs().sum() + abs(loss0))
    return {"lse": (lse, E_lse), "loss": (loss, E_loss)}


def ce_rows_bwd(logits, labels, lse, gout, weight, k_exp=None):
    """lse is the kernel's fp32 input -> {dlogits}."""
    k_exp = K_EXP if k_exp is None else k_exp
    z = logits.double()
    rows, C = z.shape
    lab = torch.arange(rows) if labels is None else labels
    g = float(f32(weight)) * (1.0 if gout is None else float(f32(gout)))
    a = z - lse.double()[:, None]
    p = torch.exp(a)
    d = g * (p - 1.0 * (torch.arange(C)[None, :] == lab[:, None]))
    return {"dlogits": (d, abs(g) * _E_p(p, a, torch.zeros_like(a), k_exp) + 3 * U * d.abs())}


def loss_reduce(lse_a, pos_a, lse_b, pos_b, coef, loss0):
    n = lse_a.shape[0]
    t = lse_a.double() - pos_a.double()
    sides = 1
    if lse_b is not None:
        t = torch.cat([t, lse_b.double() - pos_b.double()])
        sides = 2
    cf = float(f32(coef))
    loss = loss0 + cf * t.sum()
    E = abs(cf) * (sides * math.ceil(n / 256) + 10) * U * t.abs().sum() + U * (abs(cf * t.sum()) + abs(loss) + abs(loss0))
    return {"loss": (loss, E)}


def cluster_mean_cols_fwd(logits, labels, k):
    """logits [n, N] (the valid columns); every cluster id in [0, k) has a member."""
    z = logits.double()
    onehot = (labels[:, None] == torch.arange(k)[None, :]).double()       # [N, k]
    cnt = onehot.sum(0)
    out = (z @ onehot) / cnt
    return {"out": (out, (cnt - 1).clamp(min=0) * U * (z.abs() @ onehot) / cnt + U * out.abs())}, cnt.to(torch.int32)


def cluster_mean_cols_bwd(dout, labels, counts):
    d = dout.double()[:, labels] / counts[labels].double()[None, :]
    return {"dlogits": (d, U * d.abs())}


def cluster_centroids(T, labels, k):
    """float64, members added in ascending j (the order matters only to fp32); an empty cluster gives a zero row."""
    out = torch.zeros(k, T.shape[1], dtype=torch.float64)
    cnt = torch.zeros(k, dtype=torch.float64)
    for j in range(T.shape[0]):
        c = int(labels[j])
        if 0 <= c < k:
            out[c] += T[j].double()
            cnt[c] += 1
    return out / cnt.clamp(min=1)[:, None]
