"""Float64 reference, exact-data regime, derived error bars and an fp32 emulation (with mutations) for the sigmoid pairwise loss:
the kernels of csrc/sigmoid_head.hip (mmg_sigmoid_rows_fwd, mmg_sigmoid_rows_bwd) and the choreography of `head.FusedSigmoidLoss`.

Imported by tests/test_sigmoid_ref_cpu.py and tests/test_sigmoid_loss_cpu.py (no GPU) and by tests/test_sigmoid_loss_gpu.py (the kernels
against the same reference).  Everything here runs on the CPU.  The reference tree has no such loss: the independent statement the
reference below is pinned against is `-logsigmoid(y z).sum() / N` with torch's float64 autograd (pinned_statement).

The operation (X [n_loc,D] local rows, Y [N,D] gathered rows, fp32, L2-normalised; s, b fp32 scalars):
    z_ij = s <X_i,Y_j> + b;  y_ij = +1 for a positive pair, else -1;  u_ij = -y_ij z_ij
    positive: col_label None ? j == diag_off + i : col_label[j] == row_key[i]
    row_loss[i] = sum_j softplus(u_ij);  loss = coef sum_i row_loss[i]
    g_ij = coef gout (-y_ij) sigmoid(u_ij);  dX = s g Y;  dscale = F_s + sum g_ij <X_i,Y_j>;  dbias = F_b + sum g_ij  (F = the pre-fill)

Bars (u = 2^-24, first order, carried through absolute values; Kd(n) = 2 n + 16 for an n-term fp32 dot product on the f32 MFMA, the
project's convention).  The kernel's summation trees are restated: a row's 16 columns of a tile per lane, ceil(tiles / 4) tiles per
wave, one half-wave exchange, four waves; T = 16 ceil(ceil(N / 32) / 4) + 3 additions at most on any term's path.
  <x,y>     E_dot = Kd(D) u sum_d |x_d||y_d|
  z         E_z = |s| E_dot + 2 u (|s <x,y>| + |b|)
  softplus  d softplus / du = sigmoid(u), increasing, so |softplus(u + e) - softplus(u)| <= sigmoid(u + E_z) E_z (never more than the
            global Lipschitz constant 1):  E_sp = sigmoid(u + E_z) E_z + K_FN u log1p(exp(-|u|)) + u softplus(u)
  sigmoid   sigma' = sigma (1 - sigma) <= min(1/4, sigma, 1 - sigma), taken at the unfavourable end of [u - E_z, u + E_z]:
            E_sig = min(1/4, sigmoid(u + E_z), sigmoid(-(u - E_z))) E_z + (K_FN + 3) u sigmoid(u)   (exp, 1 + e, the division)
  g         E_g = |coef gout| E_sig + 3 u |g|                      (coef as fp32, its product with gout, the product with sigma)
  row_loss  sum_j E_sp + T u sum_j softplus
  loss      coef (sum_i E_row + (ceil(n / 256) + 8) u sum_i row_loss) + (2 + ranks) u |loss|
  dX        |s| (E_g |Y| + Kd(N) u |g||Y|) + u |dX|               (|.| |Y|: the matrix product of absolute values)
  dscale    sum (E_g |dot| + |g| E_dot + u |g dot|) + A u (sum |g dot| + |F|)
  dbias     sum E_g + A u (sum |g| + |F|)
            A = T + 6 + 3 + blocks + ranks + 1: the lane's terms, the wave butterfly, the four waves, one float atomic per workgroup
            (bounded for ANY order: no term passes more than `blocks` of them), the sum over ranks, the pre-fill.
K_FN is measured, not derived: the accuracy in ulps of the device's expf / log1pf is not in the code.  See K_FN below.

Exact regime (exact_case): one-hot rows, s = 256, b = -128, coef and gout powers of two.  <X_i,Y_j> is 0 or 1, every z is +-128,
e^-128 = 2^-184.7 is far below half the smallest fp32 subnormal (2^-150) and rounds to 0, so softplus is exactly 0 or 128 and
sigmoid exactly 0 or 1 (float64 keeps the 3e-56, which the checks below allow for); every sum is a sum of equal dyadic terms below 2^24 of them.  exactness_violations() asserts this on the
reference alone.

The emulation (emulate) is the kernels' arithmetic in fp32 torch on tiles padded as clip_tile.h pads them (rows >= n_loc and columns
>= N are clamped duplicates of the last valid one, then selected to zero); emulate_loss is the host choreography over simulated ranks.
MUTATIONS / HOST_MUTATIONS break one thing at a time."""
import math
import types

import torch

U = 2.0 ** -24
# Accuracy of the device's expf / log1pf in ulps.  Measured against the float64 reference with K_FN = 1 on the MI355X by
# tests/test_sigmoid_loss_gpu.py (the rows with "k_fn": 1 of profiles/sigmoid_measured_tolerances.jsonl): the worst ratio of any output
# in any case was 0.1003 (dX at (31, 31, 32), clusters); the rule - the smallest power of two that is at least 4 times the worst
# ratio, 0.401 - gives 0.5.  The bars are dominated by E_z (the fp32 dot product), so the measurement bounds K_FN only loosely from
# above; 0.5 ulp is what a correctly rounded function has, and the rows with "k_fn": 0.5 are the ratios under the constant as set.
K_FN = 0.5
COLS_PER_PASS = 128          # columns one workgroup pass covers in csrc/sigmoid_head.hip: 4 waves x one 32-column tile
EXACT_S, EXACT_B = 256.0, -128.0
SB_PAIRS = ((10.0, -10.0), (14.2857, 0.0), (100.0, -12.0))


# (n_loc, N, D, diag_off): the smallest shapes at which the tiling can go wrong - one pair; one partial tile; one tile and one row /
# column more; three row tiles and the widest D (the NDT = 8 backward); one column more than a workgroup pass; a rank that is not
# the first.  D = 32 / 64 / 512 / 1024 take the NDT = 1 / 1 / 4 / 8 instantiations of the backward; (34, 35, 256) and (33, 33, 256)
# are there for NDT = 2.
SHAPES = ((1, 1, 32, 0), (31, 31, 32, 0), (33, 33, 64, 0), (65, 65, 1024, 0), (32, COLS_PER_PASS + 1, 512, 0), (32, 96, 64, 64),
          (34, 35, 256, 0), (33, 33, 256, 0))
MODES = ("diagonal", "clusters")


def keys_for(mode, n_loc, N, diag_off):
    """(row_key, col_label) of a kernel-level case: None, None for the diagonal; hand-made cluster ids otherwise."""
    if mode == "diagonal":
        return None, None
    col_label = hand_labels(N)
    return col_label[diag_off:diag_off + n_loc].clone(), col_label


def Kd(n):
    return 2 * n + 16


def f32(v):
    """The fp32 value of a Python number, as a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


def positive_mask(n_loc, N, diag_off=0, row_key=None, col_label=None):
    if col_label is None:
        return (torch.arange(N)[None, :] == (diag_off + torch.arange(n_loc))[:, None])
    return col_label[None, :] == row_key[:, None]


def softplus64(u):
    return u.clamp(min=0) + torch.log1p(torch.exp(-u.abs()))


def reference(X, Y, s, b, pos, coef=1.0, gout=1.0, dscale0=0.0, dbias0=0.0, k_fn=None, ranks=1):
    """float64 values and bars from fp32 X [n,D], Y [N,D], the fp32 values s, b and the boolean positives [n,N]."""
    k_fn = K_FN if k_fn is None else k_fn
    n, D = X.shape
    N = Y.shape[0]
    Xd, Yd = X.double(), Y.double()
    s, b, coef, gout = float(s), float(b), float(coef), float(gout)
    dot, adot = Xd @ Yd.t(), Xd.abs() @ Yd.abs().t()
    z = s * dot + b
    ysign = torch.where(pos, 1.0, -1.0).double()
    u = -ysign * z
    sp, sig = softplus64(u), torch.sigmoid(u)
    c_up = coef * gout
    g = c_up * (-ysign) * sig
    r = types.SimpleNamespace(dot=dot, z=z, u=u, sp=sp, sig=sig, g=g, n=n, N=N, D=D)
    r.row_loss = sp.sum(1)
    r.loss = coef * r.row_loss.sum()
    r.dX = s * (g @ Yd)
    r.dscale = dscale0 + (g * dot).sum()
    r.dbias = dbias0 + g.sum()
    # ---- bars
    T = 16 * math.ceil(math.ceil(N / 32) / 4) + 3
    blocks = math.ceil(n / 32)
    A = T + 6 + 3 + blocks + ranks + 1
    E_dot = Kd(D) * U * adot
    E_z = abs(s) * E_dot + 2 * U * ((s * dot).abs() + abs(b))
    E_sp = torch.sigmoid(u + E_z) * E_z + k_fn * U * torch.log1p(torch.exp(-u.abs())) + U * sp
    lip = torch.minimum(torch.minimum(torch.sigmoid(u + E_z), torch.sigmoid(-(u - E_z))), torch.full_like(u, 0.25))
    E_sig = lip * E_z + (k_fn + 3) * U * sig
    E_g = abs(c_up) * E_sig + 3 * U * g.abs()
    r.E_z, r.E_sp, r.E_g = E_z, E_sp, E_g
    r.E_row_loss = E_sp.sum(1) + T * U * sp.sum(1)
    r.E_loss = coef * (r.E_row_loss.sum() + (math.ceil(n / 256) + 8) * U * r.row_loss.sum()) + (2 + ranks) * U * abs(r.loss)
    r.E_dX = abs(s) * (E_g @ Yd.abs() + Kd(N) * U * (g.abs() @ Yd.abs())) + U * r.dX.abs()
    r.E_dscale = (E_g * dot.abs() + g.abs() * E_dot + U * (g * dot).abs()).sum() + A * U * ((g * dot).abs().sum() + abs(dscale0))
    r.E_dbias = E_g.sum() + A * U * (g.abs().sum() + abs(dbias0))
    return r


def reference_loss(img, txt, s, b, labels=None, gout=1.0, k_fn=None, ranks=1):
    """The loss of the GLOBAL batch (img, txt: [N,D] fp32 normalised rows of all ranks) and its gradients, float64, with bars:
    loss, dimg, dtxt, dscale, dbias and E_*.  labels None = the diagonal."""
    N = img.shape[0]
    pos = positive_mask(N, N, 0, labels, labels)
    a = reference(img, txt, s, b, pos, 1.0 / N, gout, k_fn=k_fn, ranks=ranks)
    t = reference(txt, img, s, b, pos.t(), 1.0 / N, gout, k_fn=k_fn, ranks=ranks)
    return types.SimpleNamespace(loss=a.loss, E_loss=a.E_loss, dimg=a.dX, E_dimg=a.E_dX, dtxt=t.dX, E_dtxt=t.E_dX, dscale=a.dscale,
                                 E_dscale=a.E_dscale, dbias=a.dbias, E_dbias=a.E_dbias, row_loss=a.row_loss, E_row_loss=a.E_row_loss, pos=pos)


def pinned_statement(img, txt, s, b, labels=None):
    """The independent statement: -logsigmoid(y z).sum() / N in float64 torch with autograd -> loss, dimg, dtxt, dscale, dbias."""
    N = img.shape[0]
    a, t = img.double().clone().requires_grad_(True), txt.double().clone().requires_grad_(True)
    sd, bd = torch.tensor(float(s), dtype=torch.float64, requires_grad=True), torch.tensor(float(b), dtype=torch.float64, requires_grad=True)
    y = torch.where(positive_mask(N, N, 0, labels, labels), 1.0, -1.0).double()
    loss = -torch.nn.functional.logsigmoid(y * (sd * (a @ t.t()) + bd)).sum() / N
    loss.backward()
    return loss.detach(), a.grad, t.grad, sd.grad, bd.grad


def ratio(got, want, bar):
    """max |got - want| / bar; where the bar is 0 the values must be equal (inf otherwise).  Non-finite `got` gives inf."""
    got = torch.as_tensor(got).double().reshape(-1)
    want, bar = torch.as_tensor(want).double().reshape(-1), torch.as_tensor(bar).double().reshape(-1)
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got - want).abs()
    q = torch.where(bar > 0, err / bar.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(q.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
def gaussian_case(n_loc, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.nn.functional.normalize(torch.randn(n_loc, D, generator=g), dim=1)
    Y = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
    return X.contiguous(), Y.contiguous()


def hand_labels(N):
    """Cluster ids of N columns, made by hand: a cluster that spans the 32-column tile seam (columns 30..33, as far as they exist), a
    singleton (column 0), and the rest in runs of three."""
    lab = torch.empty(N, dtype=torch.int64)
    nxt = 0
    j = 0
    while j < N:
        if j == 0:
            width = 1
        elif j == 30:
            width = 4
        else:
            width = min(3, 30 - j) if j < 30 else 3
        lab[j:j + width] = nxt
        nxt += 1
        j += width
    return lab


def exact_case(n_loc, N, D, diag_off, clusters):
    """One-hot unit rows: X_i = e_{a_i}, Y_j = e_{c_j}; <X_i,Y_j> = [a_i == c_j], z = +-128 with s = 256, b = -128.  A pair is
    classified correctly iff [a_i == c_j] equals [positive].  With m = min(D, 4) directions and every fifth column shifted by one,
    positives and negatives are misclassified both ways as soon as there are more than m columns."""
    m = min(D, 4)
    gi = diag_off + torch.arange(n_loc)
    j = torch.arange(N)
    a = gi % m
    c = torch.where(j % 5 == 0, (j + 1) % m, j % m)
    X = torch.zeros(n_loc, D)
    Y = torch.zeros(N, D)
    X[torch.arange(n_loc), a] = 1.0
    Y[j, c] = 1.0
    if clusters:
        col_label = hand_labels(N)
        row_key = col_label[gi.clamp(max=N - 1)].clone()
    else:
        col_label = row_key = None
    return X, Y, row_key, col_label


def exactness_violations(r, pos, coef, gout, dscale0, dbias0):
    """Preconditions of the exact regime, on the reference alone: |z| = 128 everywhere; both kinds of pair misclassified (more than 4
    columns); every output a dyadic sum below 2^24 units.  Returns a list of complaints (empty = exact comparison is justified)."""
    bad = []
    if not bool((r.z.abs() == 128.0).all()):
        bad.append("|z| != 128")
    wrong = r.u > 0
    if r.N > 4 and not (bool((wrong & pos).any()) and bool((wrong & ~pos).any())):
        bad.append("positives and negatives are not both misclassified")
    unit = abs(coef * gout)
    if math.frexp(unit)[0] != 0.5 or math.frexp(gout)[0] != 0.5:
        bad.append("coef * gout is not a power of two")
    acc = min(unit, 2.0 ** -8)          # the accumulated scalars: the terms and the pre-fill (a multiple of 2^-8) share this quantum
    for name, v, q in (("row_loss", r.row_loss, 128.0), ("dX", r.dX, unit * EXACT_S), ("dscale", torch.stack([r.dscale, torch.tensor(dscale0).double()]), acc),
                       ("dbias", torch.stack([r.dbias, torch.tensor(dbias0).double()]), acc)):
        k = v / q
        if not bool(((k - k.round()).abs() * q < 1e-50).all()) or float(k.abs().max()) >= 2 ** 24:      # (float64 keeps exp(-128) = 3e-56)
            bad.append(f"{name} is not a dyadic sum below 2^24 units")
    cnt = wrong.sum().item() * unit / acc + max(abs(dscale0), abs(dbias0)) / acc
    if cnt >= 2 ** 24:
        bad.append("too many terms")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# emulation of the kernels (fp32 torch) and its mutations
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("no_bias", "pos_sign", "no_diag_off", "label_vs_index", "pad_col", "pad_row", "no_coef_dbias", "naive_softplus")


def _pad_to(t, rows):
    if t.shape[0] == rows:
        return t
    return torch.cat([t, t[-1:].expand(rows - t.shape[0], *t.shape[1:])])


def emulate(X, Y, s, b, row_key=None, col_label=None, diag_off=0, coef=1.0, gout=None, dscale0=None, dbias0=None, mut=None):
    """-> row_loss [n], dX [n,D], dscale, dbias (fp32 tensors; the scalars None when their pre-fill is None), computed on padded tiles."""
    assert mut is None or mut in MUTATIONS, mut
    n, D = X.shape
    N = Y.shape[0]
    np_, Np = 32 * math.ceil(n / 32), 32 * math.ceil(N / 32)
    Xp, Yp = _pad_to(X.float(), np_), _pad_to(Y.float(), Np)
    s32, b32 = torch.tensor(s, dtype=torch.float32), torch.tensor(0.0 if mut == "no_bias" else b, dtype=torch.float32)
    dot = Xp @ Yp.t()
    z = dot * s32 + b32
    ig = torch.arange(np_)
    jg = torch.arange(Np)
    off = 0 if mut == "no_diag_off" else diag_off
    if col_label is None:
        pos = jg[None, :] == (off + ig)[:, None]
    else:
        rk = (diag_off + ig) if mut == "label_vs_index" else _pad_to(row_key, np_)
        pos = _pad_to(col_label, Np)[None, :] == rk[:, None]
    valid = torch.ones(np_, Np, dtype=torch.bool)
    if mut != "pad_col":
        valid &= (jg < N)[None, :]
    valid_fwd = valid.clone()
    if mut != "pad_row":
        valid &= (ig < n)[:, None]
    ysign = torch.where(pos, 1.0, -1.0)
    if mut == "pos_sign":
        ysign = -torch.ones_like(ysign)
    u = -ysign * z
    e = torch.exp(-u.abs())
    sp = torch.log(1.0 + torch.exp(u)) if mut == "naive_softplus" else u.clamp(min=0) + torch.log1p(e)
    row_loss = torch.where(valid_fwd, sp, torch.zeros_like(sp)).sum(1)[:n]
    sig = torch.where(u >= 0, torch.ones_like(e), e) / (1.0 + e)
    c_up = torch.tensor(coef, dtype=torch.float32) * torch.tensor(1.0 if gout is None else gout, dtype=torch.float32)
    g = torch.where(valid, -ysign * c_up * sig, torch.zeros_like(sig))
    dX = ((g @ Yp) * s32)[:n]
    dscale = None if dscale0 is None else torch.tensor(dscale0, dtype=torch.float32) + (g * dot).sum()
    gb = g / c_up if mut == "no_coef_dbias" else g
    dbias = None if dbias0 is None else torch.tensor(dbias0, dtype=torch.float32) + gb.sum()
    return row_loss, dX, dscale, dbias


class TorchSigmoidBackend:
    """`head._HipSigmoidBackend` restated with emulate(): what the CPU / gloo tests install in its place."""

    @staticmethod
    def rows_forward(x_loc, y_all, scale, bias, row_key, col_label, diag_off):
        return emulate(x_loc, y_all, float(scale), float(bias), row_key, col_label, diag_off)[0]

    @staticmethod
    def loss_sum(row_loss, coef):
        return (torch.tensor(coef, dtype=torch.float32) * row_loss.sum()).reshape(1)

    @staticmethod
    def rows_backward(x_loc, y_all, scale, bias, row_key, col_label, gout, coef, diag_off, dscale=None, dbias=None):
        _, dx, ds, db = emulate(x_loc, y_all, float(scale), float(bias), row_key, col_label, diag_off, coef, float(gout),
                                None if dscale is None else 0.0, None if dbias is None else 0.0)
        if dscale is not None:
            dscale += ds
        if dbias is not None:
            dbias += db
        return dx


HOST_MUTATIONS = ("scalars_twice", "norm_n_loc")


def emulate_loss(img, txt, s, b, labels=None, world=1, gout=1.0, mut=None):
    """The choreography of head.FusedSigmoidLoss over `world` simulated ranks, in fp32 on emulate(): -> loss, dimg, dtxt, dscale, dbias
    of the global batch (the scalars summed over the ranks, as GradSync does)."""
    assert mut is None or mut in HOST_MUTATIONS, mut
    N = img.shape[0]
    nl = N // world
    coef = 1.0 / (nl if mut == "norm_n_loc" else N)
    loss = torch.zeros((), dtype=torch.float32)
    dimg, dtxt = [], []
    dscale, dbias = torch.zeros((), dtype=torch.float32), torch.zeros((), dtype=torch.float32)
    for r in range(world):
        sl = slice(r * nl, (r + 1) * nl)
        key = None if labels is None else labels[sl]
        row_loss, di, ds, db = emulate(img[sl], txt, s, b, key, labels, r * nl, coef, gout, 0.0, 0.0)
        loss = loss + torch.tensor(coef, dtype=torch.float32) * row_loss.sum()
        _, dt, ds2, db2 = emulate(txt[sl], img, s, b, key, labels, r * nl, coef, gout, 0.0, 0.0)
        dimg.append(di)
        dtxt.append(dt)
        dscale, dbias = dscale + ds, dbias + db
        if mut == "scalars_twice":
            dscale, dbias = dscale + ds2, dbias + db2
    return loss, torch.cat(dimg), torch.cat(dtxt), dscale, dbias
