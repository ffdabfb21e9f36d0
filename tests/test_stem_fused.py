"""The fused stem launches of csrc/stem.hip (mmg_stem_fwd, mmg_stem_bwd) against a float64 reference with derived error bars, their exact
cases, their accumulate semantics, the MMG_STEM_FUSED knob in the tower, and (no GPU) their argument validation.

The operation, with the roundings of the three-launch path it replaces (gemm_nt -> s0 bf16, layernorm_fwd; layernorm_bwd -> ds0 bf16,
gemm_tn_acc):
    forward   s0 = bf16(p0 w^T + bias);  mean, var = row statistics of s0;  rstd = (var + eps)^-1/2;  x = bf16((s0 - mean) rstd gamma + beta)
    backward  (mean, rstd are fp32 INPUTS)  xhat = (s0 - mean) rstd;  g = dx gamma;  ds0 = bf16(rstd (g - mean(g) - xhat mean(g xhat)))
              dW += ds0^T p0;  db += colsum(ds0);  ln_dw += sum_rows dx xhat;  ln_db += colsum(dx)

Data.  A bf16 rounding in the MIDDLE of a chain is a step function: wherever the fp32 product lands on the other side of a rounding boundary
than the float64 product, s0 differs by a whole bf16 ulp and the row's LayerNorm with it.  So the product is made EXACT: p0 in k/16
(|k| <= 16), w in k/8 (|k| <= 8), bias in k/128 - every partial sum of p0 w^T + bias is a multiple of 2^-7 below 2^10 and fp32 adds them
without error in any order.  s0 is then the same bits in the reference and in both paths (asserted on the reference alone), and it still
needs its rounding: the sums reach +-16, where the bf16 grid is 2^-4.  ds0 has no such regime (it follows a LayerNorm); its rounding
is handled in the bars (below).  Rows are periodic (row i = base row i mod 257): the reference is computed for at most 257 rows, equal rows
must give equal bits, the accumulated outputs weigh a base row by its count.

Bars (u = 2^-24, hulp = half a bf16 ulp at the reference; first order, through absolute values; the derivation of
tests/layernorm_ref.py with this kernel's sums).  A row sum adds 4 C/16 elements in a lane and then 2 butterfly steps (forward), or C/16
and then 4 (backward): D = 4 C/16 + 2 bounds the additions any term passes in either, and in the plain LayerNorm kernels too.
  mean      E_mean = (D + 2) u mean|s0|
  rstd      1/2 rstd^3 (2 mean|d| E_mean + E_mean^2 + (D + 6) u (var + eps)) + K_RSQ u rstd,  d = s0 - mean
  x         hulp + |gamma| (rstd (E_mean + 2 u |d|) + |d| E_rstd) + 2 u (|xhat gamma| + |beta|)
  ds0       (not an output) E_ds = rstd E_t + u |ds0|, E_t as layernorm_ref derives it.  The kernel's bf16(ds0) equals the reference's
            unless the float64 value lies within E_ds of a rounding boundary (amb = [bf16(ds0 - E_ds) != bf16(ds0 + E_ds)], from the
            reference alone), and then it is the neighbouring bf16 value: one ulp.
  dW        sum_r amb ulp(ds0) |p0| + k u (sum_r |ds0| |p0| + |F|);   db: the same with |p0| = 1;   F = the pre-fill
  ln_dw     sum_r |dx| 2 u |xhat| + k u (sum_r |dx xhat| + |F|);      ln_db: k u (sum_r |dx| + |F|)
            k = 32 steps-per-wave + 4 + workgroups + 2: the additions of the levels of the accumulation (a wave's rows, the LDS atomics of the
            four waves, the global atomics of the grid), each bounded for ANY order of its additions.
K_RSQ (the accuracy of the device rsqrtf, not in the code) is tests/layernorm_ref.py's: measured on the LayerNorm kernels, which are the
three-launch path.  Nothing here was calibrated on the fused kernels; what they measure goes to tests.conftest.measured (committed copy:
profiles/stem_measured_tolerances.jsonl; first MI355X run: every exact case exact, worst ratios x 0.999 - the half ulp of its own rounding -,
dW 0.975 and db 0.943 - where a ds0 sat on a rounding boundary -, rstd 0.11, everything else below 0.06)."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

from mmgclip import _hip
from tests import layernorm_ref as R
from tests.conftest import measured

gpu = pytest.mark.gpu
BF, F64, F32 = torch.bfloat16, torch.float64, torch.float32
U = 2.0 ** -24
EPS = 1e-6
P = 257                                            # period of the rows
CONFIGS = ((96, 32), (96, 64), (128, 32))
FILL = {"dW": 0.5, "db": -3.0, "ln_dw": 0.25, "ln_db": -1.5}
EXTRA = 64                                         # sentinel rows behind every [M, ...] output
SENT = {BF: (torch.int16, 0x5A5A), F32: (torch.int32, 0x5A5A5A5A)}
NANB = {BF: 0x7FC1, F32: 0x7FC00001}
FWD_WPS = {(96, 32): 3}                            # workgroups per CU of the forward (csrc/stem.hip; every other width: 2)
BWD_WPS = {(96, 32): 2}                            #                 ... of the backward (every other width: 1)


def _rb(t):
    return t.to(F32).to(BF).to(F64)


def _r32(t):
    return t.to(F32).to(F64)


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _sync():
    """A GPU fault ends the run: nothing more is started on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, stopping: {e}", returncode=3)


def _sizes(dev, C, kp):
    """The issue's four sizes and the one at which every workgroup of BOTH launches' grids walks its loop at least twice, plus a tail."""
    cu = _cus(dev)
    twice = 2 * cu * max(FWD_WPS.get((C, kp), 2) * 256, BWD_WPS.get((C, kp), 1) * 128) + 37
    return {"tile": 64, "tail": 99, "row": 1, "cu2": 2 * cu * 64 + 37, "twice": twice}


SIZE_NAMES = ("tile", "tail", "row", "cu2", "twice")


# ---- data, reference, bars (CPU, float64) -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=16)
def _data(C, kp, n, seed=0):
    g = torch.Generator().manual_seed(1000 * C + 10 * kp + n + seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(F64)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    d = SimpleNamespace(C=C, kp=kp, n=n)
    d.p0, d.w, d.bias = ri(-16, 16, n, kp) / 16, ri(-8, 8, C, kp) / 8, ri(-16, 16, C) / 128
    d.gamma, d.beta = _r32(1 + 0.2 * rn(C)), _r32(0.1 * rn(C))
    d.dx = _rb(0.5 * rn(n, C))
    return _reference(d)


def _reference(d):
    """Adds the float64 forward and backward of the n base rows and their per-element bars to d."""
    A = torch.abs
    C = d.C
    D = 4 * (C // 16) + 2
    prod = d.p0 @ d.w.T + d.bias
    # the exact-product regime, on the reference alone: multiples of 2^-7, every partial sum below 2^10
    assert torch.equal(prod * 128, torch.round(prod * 128)) and float((A(d.p0) @ A(d.w).T + A(d.bias)).max()) < 2.0 ** 10
    assert torch.equal(_rb(d.p0), d.p0) and torch.equal(_rb(d.w), d.w)
    s0 = d.s0 = _rb(prod)
    assert not torch.equal(s0, prod), "no product needs its bf16 rounding"
    mean = s0.mean(1)
    dv = s0 - mean[:, None]
    var = (dv * dv).mean(1)
    rstd = (var + EPS) ** -0.5
    xhat = dv * rstd[:, None]
    y = xhat * d.gamma + d.beta
    e_mean = (D + 2) * U * A(s0).mean(1)
    e_rstd = 0.5 * rstd ** 3 * (2 * A(dv).mean(1) * e_mean + e_mean ** 2 + (D + 6) * U * (var + EPS)) + R.K_RSQ * U * rstd
    e_xhat = rstd[:, None] * (e_mean[:, None] + 2 * U * A(dv)) + A(dv) * e_rstd[:, None]
    d.fwd = dict(x=y, mean=mean, rstd=rstd)
    d.fwd_bar = dict(x=R.half_ulp_bf16(y) + A(d.gamma) * e_xhat + 2 * U * (A(xhat * d.gamma) + A(d.beta)), mean=e_mean, rstd=e_rstd)
    # backward: the statistics are fp32 inputs
    d.mean32, d.rstd32 = _r32(mean), _r32(rstd)
    _backward_reference(d, d.dx, d.mean32, d.rstd32)
    return d


def _backward_reference(d, dx, mean32, rstd32):
    A = torch.abs
    D = 4 * (d.C // 16) + 2
    mu, rs = mean32[:, None], rstd32[:, None]
    xh = (d.s0 - mu) * rs
    g = dx * d.gamma
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    t = g - m1 - xh * m2
    ds = rs * t
    e_xh, e_g = 2 * U * A(xh), U * A(g)
    e_m1 = e_g.mean(1, keepdim=True) + (D + 2) * U * A(g).mean(1, keepdim=True)
    e_m2 = (e_g * A(xh) + A(g) * e_xh).mean(1, keepdim=True) + (D + 3) * U * A(g * xh).mean(1, keepdim=True)
    e_t = e_g + e_m1 + A(xh) * e_m2 + A(m2) * e_xh + 3 * U * (A(g) + A(m1) + A(xh * m2))
    e_ds = rs * e_t + U * A(ds)
    lo, hi = _rb(ds - e_ds), _rb(ds + e_ds)
    d.bwd_rows = dict(dsb=_rb(ds), flip=(hi - lo), xh=xh, e_xh=e_xh, dx=dx)      # flip: 0, or the ulp between the two candidates
    return d


def _counts(M, n):
    return torch.bincount(torch.arange(M) % n, minlength=n).to(F64)


def _bwd_totals(d, M, k, weights=None, fill=FILL):
    """The four accumulated outputs of a launch over M periodic rows (or over the rows `weights` counts) and their bars."""
    A = torch.abs
    b = d.bwd_rows
    w = (_counts(M, d.n) if weights is None else weights)[:, None]
    ref = dict(dW=(w * b["dsb"]).T @ d.p0 + fill["dW"], db=(w * b["dsb"]).sum(0) + fill["db"],
               ln_dw=(w * b["dx"] * b["xh"]).sum(0) + fill["ln_dw"], ln_db=(w * b["dx"]).sum(0) + fill["ln_db"])
    ku = k * U
    bar = dict(dW=(w * b["flip"]).T @ A(d.p0) + ku * ((w * A(b["dsb"])).T @ A(d.p0) + abs(fill["dW"])),
               db=(w * b["flip"]).sum(0) + ku * ((w * A(b["dsb"])).sum(0) + abs(fill["db"])),
               ln_dw=(w * A(b["dx"]) * b["e_xh"]).sum(0) + ku * ((w * A(b["dx"] * b["xh"])).sum(0) + abs(fill["ln_dw"])),
               ln_db=ku * ((w * A(b["dx"])).sum(0) + abs(fill["ln_db"])))
    return ref, bar


def _k_bwd(M, C, kp, cu):
    """Additions per level of the backward's accumulation (csrc/stem.hip: 32-row steps, 4 waves, grid = min(ceil(M / 128), CUs x BWD_WPS))."""
    blocks = min(-(-M // 128), cu * BWD_WPS.get((C, kp), 1))
    steps = -(-(-(-M // 32)) // (4 * blocks))
    return 32 * steps + 4 + blocks + 2


def _ratio(got, ref, bar):
    diff = (got - ref).abs()
    assert torch.isfinite(got).all()
    return torch.where(diff == 0, torch.zeros_like(diff), diff / bar).max().item()


# ---- device buffers ---------------------------------------------------------------------------------------------------------------
class Out:
    """[rows + EXTRA (, cols)] output: NaN bits in the rows the kernel owns, sentinel bits behind them."""

    def __init__(self, dtype, rows, cols, dev):
        it, tail = SENT[dtype]
        self.rows = rows
        self.raw = torch.full((rows + EXTRA, cols) if cols else (rows + EXTRA,), tail, dtype=it, device=dev)
        self.raw[:rows] = NANB[dtype]
        self.t = self.raw.view(dtype)
        self.tail = tail

    @property
    def body(self):
        return self.t[:self.rows]

    def intact(self):
        return bool((self.raw[self.rows:] == self.tail).all())


def _dev(t, dtype, dev, src=None):
    t = t.to(F32).to(dtype).to(dev)
    return (t if src is None else t[src]).contiguous()


def _fwd(d, M, dev, stats=True):
    src = (torch.arange(M) % d.n).to(dev)
    x = Out(BF, M, d.C, dev)
    mean, rstd = (Out(F32, M, 0, dev), Out(F32, M, 0, dev)) if stats else (None, None)
    args = [_dev(d.p0, BF, dev, src), _dev(d.w, BF, dev), _dev(d.bias, F32, dev), _dev(d.gamma, F32, dev), _dev(d.beta, F32, dev)]
    _sync()
    _hip.call("mmg_stem_fwd", *[_hip.ptr(a) for a in args], EPS, _hip.ptr(x.t), _hip.ptr(mean.t if stats else None),
              _hip.ptr(rstd.t if stats else None), M, d.C, d.kp, _hip.stream())
    _sync()
    return x, mean, rstd, src


def _bwd(d, M, dev, dx=None, rows=None, acc=None, fill=FILL):
    """One mmg_stem_bwd launch over the periodic rows `rows` (default: 0 .. M-1) -> the four accumulators (created with the pre-fill)."""
    src = ((torch.arange(M) if rows is None else rows) % d.n).to(dev)
    m = len(src)
    if acc is None:
        acc = {k: torch.full((d.C, d.kp) if k == "dW" else (d.C,), fill[k], dtype=F32, device=dev) for k in FILL}
    args = [_dev(d.dx if dx is None else dx, BF, dev, src), _dev(d.p0, BF, dev, src), _dev(d.w, BF, dev), _dev(d.bias, F32, dev),
            _dev(d.gamma, F32, dev), _dev(d.mean32, F32, dev, src), _dev(d.rstd32, F32, dev, src)]
    _sync()
    _hip.call("mmg_stem_bwd", *[_hip.ptr(a) for a in args], *[_hip.ptr(acc[k]) for k in ("dW", "db", "ln_dw", "ln_db")], m, d.C, d.kp,
              _hip.stream())
    _sync()
    return acc


# ---- 1. against float64 -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("size", SIZE_NAMES)
@pytest.mark.parametrize("C,kp", CONFIGS)
def test_forward_against_float64(dev, C, kp, size):
    """x, mean and rstd inside their bars; rows that are equal give equal bits; nothing is written behind row M; and the launch with
    mean = rstd = NULL (a pass that saves nothing) writes the same x, bit for bit."""
    M = _sizes(dev, C, kp)[size]
    d = _data(C, kp, min(M, P))
    x, mean, rstd, src = _fwd(d, M, dev)
    got = dict(x=x, mean=mean, rstd=rstd)
    assert all(o.intact() for o in got.values()), "a row behind M was written"
    worst = {}
    for name, o in got.items():
        assert torch.equal(o.raw[:M], o.raw[:d.n][src]), f"{name}: equal rows, different bits"
        worst[name] = _ratio(o.body[:d.n].cpu().to(F64), d.fwd[name], d.fwd_bar[name])
    measured(f"stem_f64_fwd-C{C}-kp{kp}-M{M}", **worst)
    assert max(worst.values()) <= 1.0, worst
    x0, _, _, _ = _fwd(d, M, dev, stats=False)
    assert x0.intact() and torch.equal(x0.raw, x.raw)


@gpu
@pytest.mark.parametrize("size", SIZE_NAMES)
@pytest.mark.parametrize("C,kp", CONFIGS)
def test_backward_against_float64(dev, C, kp, size):
    """The four gradients, accumulated onto a non-zero pre-fill, inside their bars."""
    M = _sizes(dev, C, kp)[size]
    d = _data(C, kp, min(M, P))
    acc = _bwd(d, M, dev)
    ref, bar = _bwd_totals(d, M, _k_bwd(M, C, kp, _cus(dev)))
    worst = {k: _ratio(acc[k].cpu().to(F64), ref[k], bar[k]) for k in FILL}
    measured(f"stem_f64_bwd-C{C}-kp{kp}-M{M}", **worst)
    assert max(worst.values()) <= 1.0, worst


# ---- 2. exact cases -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M", [64, 99, 1])
@pytest.mark.parametrize("C,kp", CONFIGS)
def test_constant_rows_give_beta_exactly(dev, C, kp, M):
    """w = 0 and a constant bias of 1/2: s0 = 1/2 in every row and column whatever p0 holds, the row sum C/2 and the mean
    (C/2) fp32(1/C) = 1/2 are exact (a power of two: the factor's rounding error cannot move it), every deviation is 0, and
    x = 0 rstd gamma + beta = bf16(beta) in every row; mean = 1/2 exactly, rstd = fp32 eps^-1/2 inside its bar."""
    g = torch.Generator().manual_seed(C + kp + M)
    p0 = (torch.randint(-16, 17, (M, kp), generator=g).to(F64) / 16).to(BF).to(dev)
    p0[M // 2] = p0[0]                                     # and a repeated row
    w = torch.zeros(C, kp, dtype=BF, device=dev)
    bias = torch.full((C,), 0.5, dtype=F32, device=dev)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(dev)
    beta = (0.1 * torch.randn(C, generator=g)).to(dev)
    from mmgclip import kernels as K
    x, mean, rstd = K.stem_fwd(p0, w, bias, gamma, beta, EPS)
    _sync()
    assert torch.equal(x, beta.to(BF)[None, :].expand(M, C))
    assert torch.equal(mean, torch.full_like(mean, 0.5))
    want = EPS ** -0.5
    assert float((rstd.double() - want).abs().max()) <= (0.5 * want ** 3 * 6 * U * EPS + R.K_RSQ * U * want) + 2.0 ** -24 * want


@gpu
@pytest.mark.parametrize("M", [64, 99, 1])
@pytest.mark.parametrize("C,kp", CONFIGS)
def test_zero_dx_leaves_the_accumulators_as_they_were(dev, C, kp, M):
    """dx = 0: ds0 = rstd (0 - 0 - xhat 0) = 0, so every gradient is exactly zero and a pre-filled accumulator keeps its bits."""
    d = _data(C, kp, min(M, P))
    acc = _bwd(d, M, dev, dx=torch.zeros_like(d.dx))
    for k, v in acc.items():
        assert torch.equal(v, torch.full_like(v, FILL[k])), k
    zero = _bwd(d, M, dev, dx=torch.zeros_like(d.dx), fill={k: 0.0 for k in FILL})
    for k, v in zero.items():
        assert not bool(v.any()), k


# ---- 3. accumulate semantics --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C,kp", CONFIGS)
def test_two_calls_on_halves_equal_one_call(dev, C, kp):
    """Rows 0 .. 63 and 64 .. 162 in two launches onto the same accumulators against one launch over all 163: both are within
    their bars of the same float64 sums (the second call starts from what the first left: the pre-fill is added to, not replaced)."""
    M, cut = 163, 64
    d = _data(C, kp, M)
    whole = _bwd(d, M, dev)
    acc = _bwd(d, M, dev, rows=torch.arange(cut))
    first = {k: v.clone() for k, v in acc.items()}
    acc = _bwd(d, M, dev, rows=torch.arange(cut, M), acc=acc)
    cu = _cus(dev)
    ref, bar = _bwd_totals(d, M, _k_bwd(M, C, kp, cu) + _k_bwd(cut, C, kp, cu))
    worst = {}
    for k in FILL:
        assert not torch.equal(first[k], acc[k]), k
        worst[k] = max(_ratio(acc[k].cpu().to(F64), ref[k], bar[k]), _ratio(whole[k].cpu().to(F64), ref[k], bar[k]))
    measured(f"stem_halves-C{C}-kp{kp}", **worst)
    assert max(worst.values()) <= 1.0, worst
    # and the first call alone is the sum over ITS rows
    w1 = torch.zeros(M, dtype=F64)
    w1[:cut] = 1
    ref1, bar1 = _bwd_totals(d, M, _k_bwd(cut, C, kp, cu), weights=w1)
    assert max(_ratio(first[k].cpu().to(F64), ref1[k], bar1[k]) for k in FILL) <= 1.0


# ---- 4. the knob, in the tower ------------------------------------------------------------------------------------------------------
@gpu
def test_knob_selects_the_path_and_both_paths_agree_in_the_tower(dev, monkeypatch):
    """ConvNeXt-T, n = 2 at 64 x 64 (M = 512 stem rows), forward and backward in one process with MMG_STEM_FUSED = 0 and = 1.  The stem's
    weights and the pixels are put into the exact-product regime (checked on patchify's rows), so s0 is the same bits on both paths and
    the float64 chain above is the reference of both: each path's x, mean and rstd must lie inside the forward bars, and each path's four
    stem gradients (as the tower's .grad holds them) inside the backward bars of the float64 backward at the dx and the statistics THAT
    path handed its stem - the two runs' dx differ wherever a bf16 x fell on the other side of a rounding boundary, so each is held
    to its own reference, with k = M + 2: any order of the M additions, whichever kernel makes them.  The tower's features are
    fp32 means of bf16 activations downstream of identical code; they are compared at the bf16 resolution, 2^-7 of the largest."""
    from mmgclip import kernels as K
    from mmgclip.networks import convnext as CN
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(11)
    tower = ConvNextTinyEncoder(micro_batch=2)
    conv, ln = tower.model.features[0][0], tower.model.features[0][1]
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-8, 9, conv.weight.shape, generator=g).float() / 8)
        conv.bias.copy_(torch.randint(-16, 17, conv.bias.shape, generator=g).float() / 128)
        ln.weight.copy_(1 + 0.2 * torch.randn(96, generator=g))
        ln.bias.copy_(0.1 * torch.randn(96, generator=g))
    tower = tower.to(dev)
    k16 = torch.randint(-16, 17, (2, 1, 64, 64), generator=g).float()
    img = ((1 + k16 / 16) / 2 if tower.scale16 else (k16 + 16) / 32).to(dev)       # scale16 maps x to 2 x - 1
    wgt = torch.randn(2, 768, generator=g).to(dev)
    p0 = K.patchify(img, 4, tower.kp, tower.scale16)
    d = SimpleNamespace(C=96, kp=tower.kp, n=512, p0=p0.cpu().to(F64), w=CN.conv_weight_rows(conv.weight.data).cpu().to(F64),
                        bias=conv.bias.data.cpu().to(F64), gamma=ln.weight.data.cpu().to(F64), beta=ln.bias.data.cpu().to(F64),
                        dx=torch.zeros(512, 96, dtype=F64))
    assert d.w.shape == (96, tower.kp)
    _reference(d)                                          # (asserts the regime)
    cap = {}
    spies = {}

    def spy(name, fn):
        spies[name] = getattr(K, name)
        monkeypatch.setattr(K, name, fn)

    def stem_fwd(*a, **kw):
        r = spies["stem_fwd"](*a, **kw)
        cap.update(fwd="fused", x=r[0].clone(), mean=r[1].clone(), rstd=r[2].clone())
        return r

    def layernorm_fwd(*a, **kw):
        r = spies["layernorm_fwd"](*a, **kw)
        if "fwd" not in cap:                               # the tower's first LayerNorm is the stem's
            cap.update(fwd="three", x=r[0].clone(), mean=r[1].clone(), rstd=r[2].clone())
        return r

    def stem_bwd(dx, *a, **kw):
        cap.update(bwd="fused", dx=dx.clone())
        return spies["stem_bwd"](dx, *a, **kw)

    def layernorm_bwd(dy, *a, **kw):
        cap.update(bwd="three", dx=dy.clone())             # (the last LayerNorm backward of the tower is the stem's)
        return spies["layernorm_bwd"](dy, *a, **kw)

    for name, fn in (("stem_fwd", stem_fwd), ("layernorm_fwd", layernorm_fwd), ("stem_bwd", stem_bwd), ("layernorm_bwd", layernorm_bwd)):
        spy(name, fn)
    names = {"dW": "features.0.0.weight", "db": "features.0.0.bias", "ln_dw": "features.0.1.weight", "ln_db": "features.0.1.bias"}
    feats, worst = {}, {}
    for knob, path in (("0", "three"), ("1", "fused"), ("0", "three")):
        monkeypatch.setenv("MMG_STEM_FUSED", knob)
        cap.clear()
        tower.zero_grad(set_to_none=True)
        feat = tower(img)
        (feat * wgt).sum().backward()
        _sync()
        assert (cap["fwd"], cap["bwd"]) == (path, path), (knob, cap["fwd"], cap["bwd"])
        feats[path] = feat.detach().double().cpu()
        for name in ("x", "mean", "rstd"):
            worst[f"{path}_{name}"] = _ratio(cap[name].cpu().to(F64), d.fwd[name], d.fwd_bar[name])
        _backward_reference(d, cap["dx"].cpu().to(F64), cap["mean"].cpu().to(F64), cap["rstd"].cpu().to(F64))
        ref, bar = _bwd_totals(d, 512, 512 + 2, fill={k: 0.0 for k in FILL})
        grads = dict(tower.model.named_parameters())
        for k, pname in names.items():
            got = grads[pname].grad.detach()
            got = CN.conv_weight_rows(got) if k == "dW" else got
            worst[f"{path}_{k}"] = _ratio(got.cpu().to(F64), ref[k], bar[k])
    measured("stem_paths_in_the_tower", **worst)
    assert max(worst.values()) <= 1.0, worst
    assert torch.isfinite(feats["fused"]).all()
    assert float((feats["fused"] - feats["three"]).abs().max()) <= 2.0 ** -7 * float(feats["three"].abs().max())


# ---- 5. argument validation (no GPU) ------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_before_any_launch():
    lib = _hip.load()
    one = ctypes.c_void_p(64)                              # any non-null pointer: validation must fail before it is read
    fwd = lambda p0=one, x=one, mean=one, rstd=one, M=64, C=96, kp=32: lib.mmg_stem_fwd(p0, one, one, one, one, EPS, x, mean, rstd, M, C, kp, None)
    bwd = lambda dx=one, dW=one, mean=one, M=64, C=96, kp=32: lib.mmg_stem_bwd(dx, one, one, one, one, mean, one, dW, one, one, one, M, C, kp, None)
    assert lib.mmg_stem_supported(96, 32) and lib.mmg_stem_supported(96, 64) and lib.mmg_stem_supported(128, 32) and lib.mmg_stem_supported(128, 64)
    for C, kp in ((192, 32), (96, 48), (96, 96), (0, 32), (97, 32)):
        assert not lib.mmg_stem_supported(C, kp)
        for f in (fwd, bwd):
            assert f(C=C, kp=kp) != 0 and b"not supported" in lib.mmg_last_error()
    for f in (fwd, bwd):
        for M in (0, -64):
            assert f(M=M) != 0 and b"must be positive" in lib.mmg_last_error()
    for bad in (dict(p0=None), dict(x=None)):
        assert fwd(**bad) != 0 and b"null pointer" in lib.mmg_last_error()
    assert fwd(mean=None) != 0 and b"both or neither" in lib.mmg_last_error()
    for bad in (dict(dx=None), dict(dW=None), dict(mean=None)):
        assert bwd(**bad) != 0 and b"null pointer" in lib.mmg_last_error()
