"""Reference of the linear probe (csrc/probe_head.hip, mmgclip/probe.py), shared by tests/test_probe_ref_cpu.py, test_probe_cpu.py and
test_probe_gpu.py.  Four parts:

  * the REFERENCE, float64 torch: `reference` = the un-normalised (L, dW, db), `objective` = F and its gradient, `reference_solver` =
    the product's own L-BFGS (`probe.lbfgs_minimize`) over the reference evaluation, so the solver itself can be held against scipy and
    sklearn.
  * the BAR, a per-element bound of |fp32 path - float64| written out as a formula (`bar`).  u = 2^-24, Kd(k) = 2 k + 16 the project's
    constant for a k-term fp32 sum on the f32 MFMA (tests/sigmoid_ref.py).  Per row i, with A_ic = sum_d |x_id||w_cd| + |b_c|:
        E_i   = Kd(D) u max_c A_ic                                   every logit of the row is within E_i of float64
        p     : |dp_ic| <= p_ic expm1(2 E_i)                          (a softmax moves by at most that under logit errors <= E_i)
                        + u / e + p_ic (Kd(C) u + (ln C + 7) u)       (the subtraction z - m enters exp with relative error
                                                                        u |z - m| and p |z - m| <= p ln(1/p) <= 1/e, sum_k p_k |z_k - m| <= ln C;
                                                                        expf within 1.5 ulp; the C-term sum; the division)
        g     : |dg_ic| <= w_i (|dp_ic| + 2 u |p_ic - [c == y_i]|)    (the subtraction and the product with w_i)
        dW    : |ddW_cd| <= sum_i |dg_ic||x_id| + Kd(R) u sum_i |g_ic||x_id| + G 2^-53 sum_i |g_ic||x_id|
                                                                       (R = 32 ceil(blocks / G) rows accumulate in one workgroup's fp32
                                                                        registers; the G partials are summed in fp64); db with x = 1
        loss  : |dl_i| <= w_i (2 E_i + (Kd(C) + ln C + 3) u + 2 u |ln s_i| + u |lse_i| + 2 u |l_i / w_i|),  |dL| <= sum_i |dl_i| + n 2^-53 sum_i |l_i|
    Nothing in it is measured on the code under test.
  * the EMULATION, fp32 torch on the CPU, of the kernel's partial structure (`emulate`, `TorchProbeBackend` = a stand-in for
    `head._HipProbeBackend`): G workgroups, workgroup g takes the 32-row blocks g, g+G, .., fp32 accumulators per workgroup, an fp64 loss
    per workgroup, the partials summed in index order in fp64.  MUTATIONS are single mistakes a kernel of this kind can make.
  * the CASES: the exact regimes (integer X in [-8,8]; W = 0 where p = 1/C exactly, and saturated integer logits where p is one-hot),
    random rows, and the seeded Gaussian blobs of the fit tests."""
import math

import numpy as np
import torch

from tests.sigmoid_ref import Kd, U

U64 = 2.0 ** -53
MAX_C = 32
AUTO_GROUPS = 256                   # the emulation's "one workgroup per CU"
MUTATIONS = ("label_off_by_one", "bias_dropped", "padded_class_admitted", "ignored_row_counted", "weight_of_predicted_class",
             "last_group_dropped", "db_wrong_column", "loss_from_zmax", "tail_rows_counted", "softmax_not_normalised")
RANDOM_SHAPES = ((33, 32, 2), (257, 96, 3), (1000, 512, 5), (200, 768, 10), (100, 1024, 32))
EXACT_NS = (1, 31, 32, 33, 200)
EXACT_GROUPS = (1, 2, 3, 0)
BLOBS = dict(n=600, D=64, C=3, l2=1e-2, seed=11)


def supported(D, C):
    return D >= 32 and D % 32 == 0 and D <= 1024 and 2 <= C <= MAX_C


def groups_of(n, n_groups, auto=AUTO_GROUPS):
    blocks = (n + 31) // 32
    return min(n_groups if n_groups > 0 else auto, blocks)


def partials_bytes(n, D, C, n_groups, auto=AUTO_GROUPS):
    return groups_of(n, n_groups, auto) * ((8 + 4 * C * (D + 1) + 7) // 8 * 8)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _row_weights(y, cw, dtype):
    valid = y >= 0
    yc = y.clamp(min=0)
    w = valid.to(dtype) if cw is None else cw.to(dtype)[yc] * valid
    return w, yc, valid


def reference(X, W, b, y, cw=None):
    """float64 (L [], dW [C,D], db [C]) and the per-row pieces the bar needs."""
    X, W, b = X.double(), W.double(), b.double()
    w, yc, _ = _row_weights(y, cw, torch.float64)
    z = X @ W.t() + b
    lse = torch.logsumexp(z, dim=1)
    p = torch.softmax(z, dim=1)
    rows = lse - z.gather(1, yc[:, None])[:, 0]
    G = p.clone()
    G[torch.arange(X.shape[0]), yc] -= 1.0
    G = G * w[:, None]
    return dict(L=(w * rows).sum(), dW=G.t() @ X, db=G.sum(dim=0), z=z, p=p, lse=lse, rows=rows, w=w, G=G, yc=yc)


def flat(L, dW, db):
    """The layout of the kernel's `out`: dW | db as [C, D+1] row-major, then L."""
    return torch.cat([torch.cat([dW, db[:, None]], dim=1).flatten(), L.reshape(1)])


def weight_sum(y, cw=None):
    return float(_row_weights(y, cw, torch.float64)[0].sum())


def objective(theta, X, y, C, l2, cw=None):
    """F = L / S + (l2 / 2) ||W||^2 and its gradient at theta = [C, D+1] flattened (numpy float64 in and out)."""
    D = X.shape[1]
    t = torch.from_numpy(np.asarray(theta, dtype=np.float64)).reshape(C, D + 1)
    r = reference(X, t[:, :D], t[:, D], y, cw)
    S = float(r["w"].sum())
    reg = t.clone()
    reg[:, D] = 0.0
    F = float(r["L"]) / S + 0.5 * l2 * float((reg * reg).sum())
    g = torch.cat([r["dW"], r["db"][:, None]], dim=1) / S + l2 * reg
    return F, g.flatten().numpy()


def reference_solver(X, y, C, l2, cw=None, max_iter=500, gtol=1e-8):
    """The product's L-BFGS over the float64 reference evaluation -> (theta, F, g, n_iter, converged, n_evaluations)."""
    from mmgclip.probe import lbfgs_minimize
    return lbfgs_minimize(lambda th: objective(th, X, y, C, l2, cw), np.zeros(C * (X.shape[1] + 1)), max_iter, gtol)


def convexity_distance(g1, g2, l2):
    """F is l2-strongly convex in W, so two points with gradients g1, g2 (float64, the W part) are at most this far apart in W."""
    return (float(np.linalg.norm(g1)) + float(np.linalg.norm(g2))) / l2


# ---- the bar -----------------------------------------------------------------------------------------------------------------------
def bar(X, W, b, y, cw=None, n_groups=0, auto=AUTO_GROUPS):
    """Per-element bound in the layout of `flat`: float64 [C (D+1) + 1]."""
    n, D = X.shape
    C = W.shape[0]
    r = reference(X, W, b, y, cw)
    Xa = X.double().abs()
    G_ = groups_of(n, n_groups, auto)
    R = 32 * (((n + 31) // 32 + G_ - 1) // G_)
    E = Kd(D) * U * (Xa @ W.double().abs().t() + b.double().abs()).max(dim=1).values                      # [n]
    p, w = r["p"], r["w"]
    dp = p * torch.expm1(2 * E)[:, None] + U / math.e + p * (Kd(C) * U + (math.log(C) + 7) * U)
    onehot = torch.zeros_like(p)
    onehot[torch.arange(n), r["yc"]] = 1.0
    dg = w[:, None] * (dp + 2 * U * (p - onehot).abs())
    Ga = r["G"].abs()
    X1 = torch.cat([Xa, torch.ones(n, 1, dtype=torch.float64)], dim=1)
    mass = Ga.t() @ X1
    dgrad = dg.t() @ X1 + Kd(R) * U * mass + G_ * U64 * mass
    lns = (r["lse"] - r["z"].max(dim=1).values).abs()
    dl = w * (2 * E + (Kd(C) + math.log(C) + 3) * U + 2 * U * lns + U * r["lse"].abs() + 2 * U * r["rows"].abs())
    dL = dl.sum() + n * U64 * (w * r["rows"]).abs().sum()
    return torch.cat([dgrad.flatten(), dL.reshape(1)])


def logit_bar(X, W, b):
    """[n] bound of every fp32 logit of a row against float64 (the E_i above)."""
    return Kd(X.shape[1]) * U * (X.double().abs() @ W.double().abs().t() + b.double().abs()).max(dim=1).values


# ---- the emulation ----------------------------------------------------------------------------------------------------------------
def emulate(X, W, b, y, cw=None, n_groups=0, mut=None, auto=AUTO_GROUPS):
    """fp32 torch in the kernel's partial structure -> float64 [C (D+1) + 1]."""
    assert mut is None or mut in MUTATIONS, mut
    n, D = X.shape
    C = W.shape[0]
    G_ = groups_of(n, n_groups, auto)
    blocks = (n + 31) // 32
    Wp = torch.zeros(32, D)
    Wp[:C] = W
    bp = torch.zeros(32)
    bp[:C] = b
    out = torch.zeros(C * (D + 1) + 1, dtype=torch.float64)
    Cs = 32 if mut == "padded_class_admitted" else C
    for g in range(G_ - 1 if mut == "last_group_dropped" and G_ > 1 else G_):
        acc = torch.zeros(32, D + 1)
        loss = torch.zeros((), dtype=torch.float64)
        for blk in range(g, blocks, G_):
            rows = torch.arange(blk * 32, blk * 32 + 32)
            inside = rows < n
            if mut == "tail_rows_counted":
                inside = torch.ones_like(inside)
            rows = rows.clamp(max=n - 1)
            xb, yb = X[rows], y[rows]
            if mut == "label_off_by_one":
                yb = torch.where(yb >= 0, (yb + 1) % C, yb)
            live = inside & (yb >= 0) & (yb < C)
            if mut == "ignored_row_counted":
                live = inside
            yc = yb.clamp(0, C - 1)
            z = xb @ Wp.t() + (0.0 if mut == "bias_dropped" else bp)
            zc = z[:, :Cs]
            m = zc.max(dim=1).values
            e = torch.exp(zc - m[:, None])
            s = e.sum(dim=1)
            p = torch.zeros(32, 32)
            p[:, :Cs] = e if mut == "softmax_not_normalised" else e / s[:, None]
            pick = p.argmax(dim=1) if mut == "weight_of_predicted_class" else yc
            wi = torch.where(live, torch.ones(32) if cw is None else cw.float()[pick], torch.zeros(32))
            gt = p.clone()
            gt[torch.arange(32), yc] -= 1.0
            gt = gt * wi[:, None]
            gt[:, Cs:] = 0.0
            zy = m if mut == "loss_from_zmax" else z[torch.arange(32), yc]
            rl = torch.where(live, wi * ((m + torch.log(s)) - zy), torch.zeros(32))
            acc[:, :D] += gt.t() @ xb
            acc[:, D] += gt.sum(dim=0)
            loss = loss + rl.double().sum()
        grad = acc[:C].clone()
        if mut == "db_wrong_column":
            grad[:, D] = acc[:C, D - 1]
        out[:C * (D + 1)] += grad.flatten().double()
        out[C * (D + 1)] += loss
    return out


def emulation(mutation=None):
    class Backend:
        """`head._HipProbeBackend` in fp32 torch on the CPU."""

        @staticmethod
        def supported(D, C):
            return supported(D, C)

        @staticmethod
        def evaluate(x, W, b, labels, class_weight=None, n_groups=0):
            return emulate(x, W, b, labels, class_weight, n_groups, mutation)
    return Backend


TorchProbeBackend = emulation()


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def integer_rows(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (n, D), generator=g).float()


def labels_for(n, C, seed, ignore_every=7):
    """Random labels in [0, C), every `ignore_every`-th row (from row 3) ignored; a single row keeps its label."""
    g = torch.Generator().manual_seed(seed + 1000)
    y = torch.randint(0, C, (n,), generator=g)
    if n > 3 and ignore_every:
        y[3::ignore_every] = -1
    return y


def pow2_weights(C):
    """Class weights that are powers of two: products with them are exact."""
    return torch.tensor([(1.0, 2.0, 0.5, 4.0)[c % 4] for c in range(C)])


def zero_weight_case(n, D, C, weighted, seed=0):
    """W = 0, b = 0: p = 1/C exactly for a power-of-two C.  -> (X, W, b, y, cw, exact dW [C,D] float64, exact db [C] float64); the
    expectations come from int64 arithmetic: 4 C g_ic = 4 w_i (1 - C [c == y_i]) is an integer."""
    assert C & (C - 1) == 0
    X, y = integer_rows(n, D, seed), labels_for(n, C, seed)
    cw = pow2_weights(C) if weighted else None
    w4 = (4 * _row_weights(y, cw, torch.float64)[0]).round().to(torch.int64)                  # 4 w_i: an integer
    onehot = torch.zeros(n, C, dtype=torch.int64)
    onehot[torch.arange(n), y.clamp(min=0)] = 1
    g4C = w4[:, None] * (1 - C * onehot)                                                      # 4 C g_ic
    dW = (g4C.t() @ X.to(torch.int64)).double() / (4 * C)
    db = g4C.sum(dim=0).double() / (4 * C)
    return X, torch.zeros(C, D), torch.zeros(C), y, cw, dW, db


def saturated_case(n, D, C, weighted, seed=0):
    """Integer logits with one winner per row at least 216 above the rest: z_ic = 256 [c == k_i] + b_c with integer 0 <= b_c <= 40
    (X[i, :C] = 8 onehot(k_i), W[c, c] = 32), so p is exactly one-hot, a correctly classified row adds exactly 0, a misclassified one
    +w_i to its winner's row of dW and -w_i to its label's, and L is an exact integer multiple of 1/2.
    -> (X, W, b, y, cw, dW, db, L) with float64 expectations from int64 arithmetic."""
    assert D >= C
    g = torch.Generator().manual_seed(seed + 7)
    X, y = integer_rows(n, D, seed), labels_for(n, C, seed)
    k = torch.randint(0, C, (n,), generator=g)
    keep = torch.rand(n, generator=g) < 0.5
    k = torch.where(keep & (y >= 0), y, k)                                                    # about half the rows are classified correctly
    X[:, :C] = 0.0
    X[torch.arange(n), k] = 8.0
    W = torch.zeros(C, D)
    W[torch.arange(C), torch.arange(C)] = 32.0
    b = torch.tensor([float((7 * c + 3) % 41) for c in range(C)])
    cw = pow2_weights(C) if weighted else None
    w2 = (2 * _row_weights(y, cw, torch.float64)[0]).round().to(torch.int64)                  # 2 w_i: an integer
    win = torch.zeros(n, C, dtype=torch.int64)
    win[torch.arange(n), k] = 1
    lab = torch.zeros(n, C, dtype=torch.int64)
    lab[torch.arange(n), y.clamp(min=0)] = 1
    g2 = w2[:, None] * (win - lab)
    bi = b.to(torch.int64)
    L2 = (w2 * (256 * (k != y) + bi[k] - bi[y.clamp(min=0)])).sum()
    return X, W, b, y, cw, (g2.t() @ X.to(torch.int64)).double() / 2, g2.sum(dim=0).double() / 2, L2.double() / 2


def random_case(n, D, C, seed=0):
    """Gaussian rows, weights and bias of a size that keeps the logits moderate, random labels with ignored rows, random positive
    class weights."""
    g = torch.Generator().manual_seed(100 + seed)
    X = torch.randn(n, D, generator=g)
    W = torch.randn(C, D, generator=g) * (1.5 / math.sqrt(D))
    b = torch.randn(C, generator=g) * 0.5
    cw = torch.rand(C, generator=g) + 0.5
    return X.contiguous(), W.contiguous(), b, labels_for(n, C, seed), cw


def blobs(n=BLOBS["n"], D=BLOBS["D"], C=BLOBS["C"], seed=BLOBS["seed"], spread=1.0):
    """Seeded Gaussian blobs: class c sits at a random centre of norm about 2, unit noise; a few rows are ignored."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(C, D, generator=g) * (2.0 / math.sqrt(D))
    y = torch.arange(n) % C
    X = centres[y] + spread * torch.randn(n, D, generator=g)
    y = y.clone()
    y[5::41] = -1
    return X.contiguous(), y
