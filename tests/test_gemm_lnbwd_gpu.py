"""mmg_gemm_nt_lnbwd (csrc/gemm_lnbwd.hip: the data-gradient GEMM with the LayerNorm backward in its epilogue) against a float64 reference
with derived error bars, its exact cases, its output semantics, its equivalence with the two launches it replaces, the MMG_LNBWD_FUSED
knob in the tower, and (no GPU) its argument validation.

The operation, with the roundings of the pair it replaces (gemm_nt -> dln bf16, layernorm_bwd):
    dln = bf16(A B^T) (fp32 accumulation);  per pixel (C consecutive columns of a row), with mean, rstd fp32 INPUTS:
    xhat = (x - mean) rstd;  g = dln gamma;  dx = bf16(rstd (g - mean_C(g) - xhat mean_C(g xhat)));  dgamma += sum dln xhat;  dbeta += sum dln
patch = 1: GEMM row r = (n, ph, pw), segment s -> pixel (n, 2 ph + s / 2, 2 pw + s % 2) of an H x W map; x, dx, mean, rstd by pixel.

Data.  A bf16 rounding in the middle of a chain is a step function, so the product is made EXACT: A in k/16 (|k| <= 16), B in k/8 (|k| <= 8):
every partial sum of A B^T is a multiple of 2^-7 below 2^17 and fp32 adds them without error in any order, at K = 1536 too (asserted on the
reference alone).  dln is then the same bits in the reference and on both paths, and it still needs its rounding (asserted: the sums reach
several units, where the bf16 grid is 2^-6 and coarser).  GEMM rows are periodic (row i = base row i mod n, n <= 257): the reference is computed
for at most 257 rows, equal rows must give equal bits, the accumulated outputs weigh a base row by its count.

Bars (u = 2^-24, hulp = half a bf16 ulp of dx at the reference; first order, through absolute values - the derivation of tests/layernorm_ref.py
with this kernel's sums).  A pixel's sum adds 24 elements in a lane and then log2(C / 24) butterfly steps: D = 24 + log2(C / 24).
    E_xh = 2 u |xhat|;  E_g = u |g|;  E_m1 = mean E_g + (D + 2) u mean|g|;  E_m2 = mean(E_g |xhat| + |g| E_xh) + (D + 3) u mean|g xhat|
    t = g - m1 - xhat m2,  E_t = E_g + E_m1 + |xhat| E_m2 + |m2| E_xh + 3 u (|g| + |m1| + |xhat m2|)
    dx       hulp + rstd E_t + u |rstd t|
    dgamma   sum_r n_r |dln| E_xh + k u (sum_r n_r |dln xhat| + |F|);   dbeta   k u (sum_r n_r |dln| + |F|);   F = the pre-fill
             k = min(pixels, 4 T + 512 / G + workgroups) + 2, the additions of the levels of the accumulation - a lane's 4 passes over each of
             the T tiles its workgroup walks, the LDS atomics of the 512 / G lanes that share a column, the global atomics of the grid - each
             bounded for ANY order of its additions.  For the pair: layernorm_bwd_plain_kernel's own levels (tests/layernorm_ref.py: plan).
Nothing here was calibrated on the new kernel; what it measures goes to tests.conftest.measured (committed copy:
profiles/lnbwd_measured_tolerances.jsonl).

The tower.  Activations there are not in the exact-product regime, so each fused site is checked where it stands: its captured inputs go
through the pair once more, the float64 LayerNorm backward of THAT dln (bf16, exact) is the reference of both, and the site's dx, dgamma and
dbeta must lie inside the bars above.  Parameter gradients of the whole backward and the gradient that reaches the stem are compared between
MMG_LNBWD_FUSED = 0 and 1 at half a bf16 ulp of the largest element (2^-9): downstream of a site both paths run identical code on what
must be the same bf16 dx up to its last bit, and fp32 atomics reorder the sums of the weight gradients from run to run on either path."""
import ctypes
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from mmgclip import _hip
from tests import layernorm_ref as R
from tests.conftest import measured

gpu = pytest.mark.gpu
BF, F64, F32 = torch.bfloat16, torch.float64, torch.float32
U = 2.0 ** -24
P = 257                                            # period of the GEMM rows
FILL = {"dgamma": 0.5, "dbeta": -3.0}
EXTRA = 64                                         # sentinel rows behind dx
SENT, NANB = 0x5A5A, 0x7FC1
BM, BN, THREADS = 128, 384, 512                    # the kernel's tile and workgroup (csrc/gemm_lnbwd.hip)
SHAPES = ((384, 64, 384, 0), (384, 192, 96, 1), (768, 384, 192, 1), (1536, 768, 384, 1), (384, 1536, 384, 0))      # (N, K, C, patch)


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


# ---- data, reference, bars (CPU, float64) -------------------------------------------------------------------------------------------
def ln_bwd_reference(dln, x, mean32, rstd32, gamma, C):
    """dln, x [n, S, C] float64 (S pixels per GEMM row), mean32 / rstd32 [n, S], gamma [C] -> SimpleNamespace of the float64 LayerNorm backward
    per pixel and its bars (module docstring)."""
    A = torch.abs
    D = 24 + int(math.log2(C // 24))
    mu, rs = mean32[..., None], rstd32[..., None]
    xh = (x - mu) * rs
    g = dln * gamma
    m1, m2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    t = g - m1 - xh * m2
    dx = rs * t
    e_xh, e_g = 2 * U * A(xh), U * A(g)
    e_m1 = e_g.mean(-1, keepdim=True) + (D + 2) * U * A(g).mean(-1, keepdim=True)
    e_m2 = (e_g * A(xh) + A(g) * e_xh).mean(-1, keepdim=True) + (D + 3) * U * A(g * xh).mean(-1, keepdim=True)
    e_t = e_g + e_m1 + A(xh) * e_m2 + A(m2) * e_xh + 3 * U * (A(g) + A(m1) + A(xh * m2))
    return SimpleNamespace(dx=dx, dx_bar=R.half_ulp_bf16(dx) + rs * e_t + U * A(dx), xh=xh, e_xh=e_xh, dln=dln)


def totals(ref, w, k, fill=FILL):
    """dgamma / dbeta of a launch whose base row i counts w[i] times, onto the pre-fill, and their bars."""
    A = torch.abs
    w = w[:, None, None]
    got = dict(dgamma=(w * ref.dln * ref.xh).sum((0, 1)) + fill["dgamma"], dbeta=(w * ref.dln).sum((0, 1)) + fill["dbeta"])
    bar = dict(dgamma=(w * A(ref.dln) * ref.e_xh).sum((0, 1)) + k * U * ((w * A(ref.dln * ref.xh)).sum((0, 1)) + abs(fill["dgamma"])),
               dbeta=k * U * ((w * A(ref.dln)).sum((0, 1)) + abs(fill["dbeta"])))
    return got, bar


@functools.lru_cache(maxsize=32)
def _data(N, K, C, n, flavour=""):
    """The n base rows of a case: exact-product A, B; x bf16, mean / rstd its fp32 statistics; the float64 reference."""
    g = torch.Generator().manual_seed(100000 * C + 10 * K + n)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(F64)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    S = N // C
    d = SimpleNamespace(N=N, K=K, C=C, n=n, S=S)
    d.a, d.b = ri(-16, 16, n, K) / 16, ri(-8, 8, N, K) / 8
    d.x = _rb(rn(n, S, C) * (1 + rn(n, S, 1).abs()) + 0.5 * rn(n, S, 1))
    d.gamma = _r32(1 + 0.2 * rn(C))
    if flavour == "constant":                      # gamma = 1, dln constant along a row (equal B rows), x constant along a pixel
        d.b = (ri(-8, 8, 1, K) / 8).expand(N, K).contiguous()
        d.x = _rb(rn(n, S, 1)).expand(n, S, C).contiguous()
        d.gamma = torch.ones(C, dtype=F64)
    prod = d.a @ d.b.T
    # the exact-product regime, on the reference alone: multiples of 2^-7, every partial sum below 2^17 (24 bits), operands on the bf16 grid
    assert torch.equal(prod * 128, torch.round(prod * 128)) and float((d.a.abs() @ d.b.abs().T).max()) < 2.0 ** 17
    assert torch.equal(_rb(d.a), d.a) and torch.equal(_rb(d.b), d.b)
    dln = _rb(prod)
    assert not torch.equal(dln, prod), "no product needs its bf16 rounding"
    mean = d.x.mean(-1)
    var = ((d.x - mean[..., None]) ** 2).mean(-1)
    d.mean32, d.rstd32 = _r32(mean), _r32((var + 1e-6) ** -0.5)
    d.ref = ln_bwd_reference(dln.reshape(n, S, C), d.x, d.mean32, d.rstd32, d.gamma, C)
    return d


def _pixels(M, N, C, patch, H, W):
    """-> pix [M, S]: the pixel (row of x, dx, mean, rstd) of segment s of GEMM row r."""
    S = N // C
    r = torch.arange(M)[:, None]
    s = torch.arange(S)[None, :]
    if not patch:
        return r.expand(M, S).contiguous()
    h2, w2 = H // 2, W // 2
    pw, ph, n = r % w2, (r // w2) % h2, r // (w2 * h2)
    return (n * H + 2 * ph + s // 2) * W + 2 * pw + s % 2


def _k_fused(M, N, C, cu):
    tiles = -(-M // BM) * (N // BN)
    grid = min(tiles, cu)
    return min(M * (N // C), 4 * -(-tiles // grid) + THREADS // (C // 24) + grid) + 2


def _k_pair(pixels, C):
    G = C // 24
    rpb = 4 * (64 // G)
    blocks = min(-(-pixels // rpb), R.CAP["bwd"])
    return min(pixels, -(-pixels // (blocks * rpb)) + rpb + blocks) + 2


def _ratio(got, ref, bar):
    diff = (got - ref).abs()
    assert torch.isfinite(got).all()
    return torch.where(diff == 0, torch.zeros_like(diff), diff / bar).max().item()


# ---- device side --------------------------------------------------------------------------------------------------------------------
class Launch:
    """The device operands of a case over M periodic rows: x, mean, rstd laid out by pixel; dx with NaN bits in the rows the kernel owns and
    sentinel bits behind them; dgamma / dbeta with the pre-fill (or absent)."""

    def __init__(self, d, M, patch, hw, dev, grads=True, fill=FILL):
        self.d, self.M, self.patch, self.hw = d, M, patch, hw
        self.src = torch.arange(M) % d.n
        self.pix = _pixels(M, d.N, d.C, patch, *hw)
        self.P = M * d.S
        assert sorted(self.pix.flatten().tolist()) == list(range(self.P))
        cast = lambda t, dt: t.to(F32).to(dt).to(dev).contiguous()
        self.a, self.b, self.gamma = cast(d.a[self.src], BF), cast(d.b, BF), cast(d.gamma, F32)
        order = torch.empty(self.P, dtype=torch.long)
        order[self.pix.flatten()] = torch.arange(self.P)           # pixel -> (row, segment) flattened
        by_pixel = lambda t: t[self.src].reshape(self.P, *t.shape[2:])[order]
        self.x, self.mean, self.rstd = cast(by_pixel(d.x), BF), cast(by_pixel(d.mean32), F32), cast(by_pixel(d.rstd32), F32)
        self.raw = torch.full((self.P + EXTRA, d.C), SENT, dtype=torch.int16, device=dev)
        self.raw[:self.P] = NANB
        self.dx = self.raw.view(BF)
        self.acc = {k: torch.full((d.C,), fill[k], dtype=F32, device=dev) for k in FILL} if grads else None

    def fused(self):
        d, g = self.d, self.acc
        _sync()
        _hip.call("mmg_gemm_nt_lnbwd", _hip.ptr(self.a), d.K, _hip.ptr(self.b), d.K, self.M, d.N, d.K, _hip.ptr(self.x), d.C, _hip.ptr(self.mean),
                  _hip.ptr(self.rstd), _hip.ptr(self.gamma), _hip.ptr(self.dx), d.C, _hip.ptr(g["dgamma"] if g else None),
                  _hip.ptr(g["dbeta"] if g else None), d.C, self.patch, self.hw[0], self.hw[1], _hip.stream())
        _sync()
        return self

    def pair(self):
        from mmgclip import kernels as K
        from mmgclip import linalg as L
        _sync()
        dln = L.gemm_nt(self.a, self.b)
        K.layernorm_bwd(dln, self.x, self.mean, self.rstd, self.gamma, self.acc["dgamma"], self.acc["dbeta"],
                        patch_hw=self.hw if self.patch else None, out=self.dx[:self.P])
        _sync()
        return self

    def intact(self):
        return bool((self.raw[self.P:] == SENT).all())

    def rows(self):
        """dx as [M, S, C] (GEMM row, segment), on the CPU."""
        return self.dx[:self.P].cpu()[self.pix.flatten()].reshape(self.M, self.d.S, self.d.C)


def _check(L, k, name):
    """dx (every base row, and equal rows equal bits), dgamma, dbeta of a finished launch against the float64 reference -> worst ratios."""
    d = L.d
    got = L.rows()
    assert L.intact(), "a row behind dx was written"
    assert torch.isfinite(got.float()).all(), "a dx element was left as it was (NaN pre-fill)"
    assert torch.equal(got.view(torch.int16), got[:d.n].view(torch.int16)[L.src]), "equal rows, different bits"
    worst = dict(dx=_ratio(got[:d.n].to(F64), d.ref.dx, d.ref.dx_bar))
    if L.acc is not None:
        ref, bar = totals(d.ref, R.counts(L.M, d.n), k)
        for key in FILL:
            worst[key] = _ratio(L.acc[key].cpu().to(F64), ref[key], bar[key])
    measured(name, **worst)
    return worst


def _cases_with(cu):
    """(id, N, K, C, patch, size tag, (H, W), images): the issue's shapes and sizes.  Plain rows: 1, 64, 99 (a tail inside a tile), 128 + 37, and
    the size at which every workgroup of the persistent grid walks its loop at least twice (K = 1536: at small M only).  Patchified rows:
    H = W in {4, 6} with 2 and 3 images, 19 images of 6 x 6 (171 rows: a tail in the second tile), and - at C = 96, the width whose x passes
    2^31 bytes in the step - the twice-round size in 6 x 6 images.  The CU count only names the cases; a launch takes the device's own."""
    twice = 2 * cu * BM + 37
    out = []
    for N, K, C, patch in SHAPES:
        if not patch:
            for tag, M in ((("row", 1), ("tile", 64), ("tail", 99), ("tiles", 165), ("twice", twice)) if K < 1536 else (("tile", 64), ("tail", 99))):
                out.append((f"N{N}-K{K}-C{C}-{tag}", N, K, C, 0, tag, (0, 0), 0))
        else:
            for hw, imgs in [(4, 2), (6, 3), (6, 19)] + ([(6, 0)] if C == 96 else []):
                out.append((f"N{N}-K{K}-C{C}-patch{hw}-img{imgs or 'twice'}", N, K, C, 1, "patch", (hw, hw), imgs))
    return out


CASES = _cases_with(256)
PAIR_CASES = [c for c in CASES if c[5] in ("tail", "tiles") or c[7] in (3, 19)]
EXACT_CASES = [c for c in CASES if c[5] == "tail" or c[7] == 3]


def _rows_of(case, dev):
    _, N, K, C, patch, tag, hw, imgs = case
    twice = 2 * _cus(dev) * BM + 37
    if not patch:
        return {"row": 1, "tile": 64, "tail": 99, "tiles": 165, "twice": twice}[tag]
    return (imgs or -(-twice // 9)) * (hw[0] // 2) ** 2


# ---- 1. against float64 -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_against_float64(dev, case):
    """dx inside its bars in every row, equal rows equal bits, the NaN pre-fill overwritten, the sentinel rows intact; dgamma and dbeta,
    accumulated onto a non-zero pre-fill, inside theirs; and the launch with dgamma = dbeta = NULL writes the same dx, bit for bit."""
    name, N, K, C, patch, _, hw, _ = case
    M = _rows_of(case, dev)
    d = _data(N, K, C, min(M, P))
    L = Launch(d, M, patch, hw, dev).fused()
    worst = _check(L, _k_fused(M, N, C, _cus(dev)), f"lnbwd_f64-{name}-M{M}")
    assert max(worst.values()) <= 1.0, worst
    L0 = Launch(d, M, patch, hw, dev, grads=False).fused()
    assert L0.intact() and torch.equal(L0.raw, L.raw)


# ---- 2. the pair, on the same inputs ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_the_pair_is_inside_the_same_bars(dev, case):
    """gemm_nt + layernorm_bwd on the operands of the fused launch: the same float64 reference, the same bars (k: the plain LayerNorm kernel's
    own levels).  Bit equality with the fused launch is not demanded (the share of dx elements that differ is recorded)."""
    name, N, K, C, patch, _, hw, _ = case
    M = _rows_of(case, dev)
    d = _data(N, K, C, min(M, P))
    Lp = Launch(d, M, patch, hw, dev).pair()
    worst = _check(Lp, _k_pair(M * d.S, C), f"lnbwd_pair-{name}-M{M}")
    assert max(worst.values()) <= 1.0, worst
    Lf = Launch(d, M, patch, hw, dev).fused()
    measured(f"lnbwd_pair_vs_fused-{name}-M{M}", dx_differ=float((Lf.raw != Lp.raw).double().mean()))


# ---- 3. exact cases -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_constant_rows_give_zero_exactly(dev, case):
    """gamma = 1, every row of B equal (dln = c_r in every column of row r) and x constant along a pixel and equal to its mean: xhat = 0, so
    mean(g xhat) = 0, and mean(g) = fl(fl(C c) fl(1 / C)) = c exactly - C = 3 * 2^j, 3 fl(1/3) = 1 + 2^-25, and c has 8 significant bits: the
    product's excess is below half an fp32 ulp - so dx = rstd (c - c - 0) = 0 in every element; dbeta = sum c_r (exact: multiples of 2^-7),
    dgamma = 0."""
    name, N, K, C, patch, _, hw, _ = case
    M = _rows_of(case, dev)
    d = _data(N, K, C, min(M, P), "constant")
    assert torch.equal(d.ref.xh, torch.zeros_like(d.ref.xh)) and bool((d.ref.dln != 0).any())
    zero = {k: 0.0 for k in FILL}
    L = Launch(d, M, patch, hw, dev, fill=zero).fused()
    assert L.intact() and not bool(L.dx[:L.P].float().any())
    assert not bool(L.acc["dgamma"].any())
    want = (R.counts(M, d.n)[:, None, None] * d.ref.dln).sum((0, 1))
    assert torch.equal(L.acc["dbeta"].cpu().to(F64), want)


# ---- 4. accumulate semantics --------------------------------------------------------------------------------------------------------
@gpu
def test_two_calls_accumulate(dev):
    """Two launches onto the same dgamma / dbeta: twice the sums on the pre-fill, inside the bars of both launches' additions."""
    N, K, C, M = 384, 64, 384, 165
    d = _data(N, K, C, M)
    L = Launch(d, M, 0, (0, 0), dev).fused()
    once = {k: v.clone() for k, v in L.acc.items()}
    L.fused()
    k = 2 * _k_fused(M, N, C, _cus(dev))
    ref, bar = totals(d.ref, 2 * R.counts(M, d.n), k)
    worst = {key: _ratio(L.acc[key].cpu().to(F64), ref[key], bar[key]) for key in FILL}
    measured("lnbwd_two_calls", **worst)
    assert max(worst.values()) <= 1.0, worst
    assert all(not torch.equal(once[key], L.acc[key]) for key in FILL)


# ---- 5. the knob, in the tower ------------------------------------------------------------------------------------------------------
def _tower_run(dev, monkeypatch, size, expect_fused_maps):
    from mmgclip import kernels as K
    from mmgclip import linalg as LA
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(size)
    tower = ConvNextTinyEncoder(micro_batch=2).to(dev)
    with torch.no_grad():                              # make the blocks matter (layer scale is 1e-6 at init)
        for n_, p in tower.named_parameters():
            if n_.endswith("layer_scale"):
                p.fill_(0.5)
    img = torch.rand(2, 1, size, size, generator=g).to(dev)
    wgt = torch.randn(2, 768, generator=g).to(dev)
    sites, stem_dx = [], {}
    real_fused, real_stem = K.gemm_nt_lnbwd, K.stem_bwd

    def spy_fused(a, b, x, mean, rstd, gamma, dgamma=None, dbeta=None, patch_hw=None, out=None):
        dx = real_fused(a, b, x, mean, rstd, gamma, dgamma, dbeta, patch_hw=patch_hw, out=out)
        sites.append(dict(a=a.clone(), b=b.clone(), x=x.clone(), mean=mean.clone(), rstd=rstd.clone(), gamma=gamma.clone(), hw=patch_hw, dx=dx.clone()))
        return dx

    def spy_stem(dx, *a, **kw):
        stem_dx["dx"] = dx.clone()
        return real_stem(dx, *a, **kw)

    monkeypatch.setattr(K, "gemm_nt_lnbwd", spy_fused)
    monkeypatch.setattr(K, "stem_bwd", spy_stem)
    grads, dxs = {}, {}
    for knob in ("0", "1"):
        monkeypatch.setenv("MMG_LNBWD_FUSED", knob)
        sites.clear()
        tower.zero_grad(set_to_none=True)
        (tower(img) * wgt).sum().backward()
        _sync()
        grads[knob] = {n_: p.grad.detach().double().cpu() for n_, p in tower.model.named_parameters() if p.grad is not None}
        dxs[knob] = stem_dx["dx"].double().cpu()
        if knob == "0":
            assert not sites, "MMG_LNBWD_FUSED=0 took the fused launch"
    assert sorted(s["hw"] for s in sites if s["hw"]) == sorted(expect_fused_maps), [s["hw"] for s in sites]
    worst = {}
    cu = _cus(dev)
    for i, s in enumerate(sites):                      # every fused site where it stands: the pair on the same inputs, float64 from its dln
        M, N, C = s["a"].shape[0], s["b"].shape[0], s["x"].shape[1]
        S, hw = N // C, s["hw"] or (0, 0)
        pix = _pixels(M, N, C, int(bool(s["hw"])), *hw).flatten()
        dln = LA.gemm_nt(s["a"], s["b"])
        acc = {p: {k: torch.zeros(C, device=dev) for k in FILL} for p in ("pair", "fused")}
        dxp = K.layernorm_bwd(dln, s["x"], s["mean"], s["rstd"], s["gamma"], acc["pair"]["dgamma"], acc["pair"]["dbeta"], patch_hw=s["hw"])
        real_fused(s["a"], s["b"], s["x"], s["mean"], s["rstd"], s["gamma"], acc["fused"]["dgamma"], acc["fused"]["dbeta"], patch_hw=s["hw"])
        _sync()
        rows = lambda t: t.cpu().to(F64)[pix].reshape(M, S, *t.shape[1:])
        ref = ln_bwd_reference(dln.cpu().to(F64).reshape(M, S, C), rows(s["x"]), rows(s["mean"]), rows(s["rstd"]), s["gamma"].cpu().to(F64), C)
        ones = torch.ones(M, dtype=F64)
        zero = {k: 0.0 for k in FILL}
        for path, dx, k in (("pair", dxp, _k_pair(M * S, C)), ("fused", s["dx"], _k_fused(M, N, C, cu))):
            tref, tbar = totals(ref, ones, k, fill=zero)
            r = dict(dx=_ratio(rows(dx), ref.dx, ref.dx_bar), **{key: _ratio(acc[path][key].cpu().to(F64), tref[key], tbar[key]) for key in FILL})
            for key, v in r.items():
                worst[f"{path}_{key}"] = max(worst.get(f"{path}_{key}", 0.0), v)
    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
    worst["param_grads"] = max(rel(grads["1"][n_], grads["0"][n_]) for n_ in grads["0"]) / 2.0 ** -9
    worst["stem_dx"] = rel(dxs["1"], dxs["0"]) / 2.0 ** -9
    assert set(grads["0"]) == set(grads["1"]) and all(torch.isfinite(v).all() for v in grads["1"].values())
    return worst, len(sites)


@gpu
def test_knob_selects_the_path_and_both_paths_agree_in_the_tower(dev, monkeypatch):
    """ConvNeXt-T, 2 images of 64 x 64, MMG_LNBWD_FUSED = 0 against 1, same dfeat (module docstring: the tower).  The maps are 16, 8 and 4
    wide: all three downsample layers take the fused launch."""
    worst, n = _tower_run(dev, monkeypatch, 64, [(16, 16), (8, 8), (4, 4)])
    measured("lnbwd_paths_in_the_tower", sites=n, **worst)
    assert max(worst.values()) <= 1.0, worst


@gpu
def test_an_odd_map_falls_back_and_both_paths_agree(dev, monkeypatch):
    """72 x 72: the stage-2 map is 9 x 9 and odd, so downsample 1 keeps the two launches (its last row and column need dx = 0 and no GEMM row
    visits them), while the 18 x 18 map of downsample 0 and the 4 x 4 map of downsample 2 take the fused one."""
    worst, n = _tower_run(dev, monkeypatch, 72, [(18, 18), (4, 4)])
    measured("lnbwd_paths_in_the_tower_72", sites=n, **worst)
    assert max(worst.values()) <= 1.0, worst


# ---- 6. argument validation (no GPU) ------------------------------------------------------------------------------------------------
SUPPORT_TABLE = (          # (N, K, C, patch, H, W) -> supported
    ((384, 64, 384, 0, 0, 0), True), ((384, 1536, 384, 0, 0, 0), True), ((384, 192, 96, 1, 256, 256), True), ((768, 384, 192, 1, 6, 4), True),
    ((1536, 768, 384, 1, 64, 64), True), ((1536, 768, 384, 1, 2, 2), True),
    ((96, 384, 96, 0, 0, 0), False), ((192, 768, 192, 0, 0, 0), False),                    # plain rows narrower than a tile
    ((383, 64, 384, 0, 0, 0), False), ((768, 64, 384, 0, 0, 0), False),                    # wrong N / N != C
    ((384, 96, 384, 0, 0, 0), False), ((384, 32, 384, 0, 0, 0), False), ((384, 0, 384, 0, 0, 0), False),       # K % 64, K < 64
    ((384, 64, 128, 0, 0, 0), False), ((384, 192, 95, 1, 4, 4), False), ((3072, 1536, 768, 1, 4, 4), False),   # C outside the set
    ((384, 192, 192, 1, 4, 4), False), ((768, 192, 96, 1, 4, 4), False),                   # N != 4 C
    ((384, 192, 96, 1, 9, 8), False), ((384, 192, 96, 1, 8, 9), False), ((384, 192, 96, 1, 0, 0), False),      # odd / missing map
    ((384, 192, 96, 2, 4, 4), False),
    # ConvNeXt-B: widths 128 / 256 / 512 / 1024 - block GEMMs N = C, downsample GEMMs N = 4 C: all fall back
    ((128, 512, 128, 0, 0, 0), False), ((256, 1024, 256, 0, 0, 0), False), ((512, 2048, 512, 0, 0, 0), False), ((1024, 4096, 1024, 0, 0, 0), False),
    ((512, 256, 128, 1, 64, 64), False), ((1024, 512, 256, 1, 32, 32), False), ((2048, 1024, 512, 1, 16, 16), False),
)


def test_bad_arguments_are_rejected_before_any_launch():
    """Every rejection with dummy pointers (validation must fail before one is read, and before any HIP call: this runs without a device);
    _supported agrees with the launch on the table - a supported shape with a NULL operand gets as far as the pointer check."""
    lib = _hip.load()
    one = ctypes.c_void_p(64)

    def launch(N, K, C, patch, H, W, M=None, A=one, dx=one, dgamma=one, dbeta=one, lda=None, ldx=None):
        M = ((H // 2) * (W // 2) * 2 or 2) if M is None else M
        return lib.mmg_gemm_nt_lnbwd(A, K if lda is None else lda, one, K, M, N, K, one, C if ldx is None else ldx, one, one, one, dx, C, dgamma, dbeta,
                                     C, patch, H, W, None)

    for shape, ok in SUPPORT_TABLE:
        assert bool(lib.mmg_gemm_nt_lnbwd_supported(*shape)) == ok, shape
        assert launch(*shape, A=None) != 0
        assert (b"null pointer" if ok else b"not supported") in lib.mmg_last_error(), (shape, lib.mmg_last_error())
    good = (384, 192, 96, 1, 6, 6)
    for M in (0, -9):
        assert launch(*good, M=M) != 0 and b"must be positive" in lib.mmg_last_error()
    for M in (1, 8, 10, 100):                          # 9 patch rows per image
        assert launch(*good, M=M) != 0 and b"not a multiple" in lib.mmg_last_error()
    assert launch(*good, dx=None) != 0 and b"null pointer" in lib.mmg_last_error()
    assert launch(*good, dbeta=None) != 0 and b"both or neither" in lib.mmg_last_error()
    assert launch(*good, dgamma=None) != 0 and b"both or neither" in lib.mmg_last_error()
    assert launch(*good, lda=128) != 0 and b"leading dimension" in lib.mmg_last_error()
    assert launch(*good, ldx=100) != 0 and b"multiples of 8" in lib.mmg_last_error()
    assert launch(*good, A=ctypes.c_void_p(72)) != 0 and b"16-byte aligned" in lib.mmg_last_error()


def test_the_python_side_agrees_with_the_library():
    from mmgclip import kernels as K
    for (N, Kd, C, patch, H, W), ok in SUPPORT_TABLE:
        if patch in (0, 1):
            assert K.gemm_nt_lnbwd_supported(N, Kd, C, (H, W) if patch else None) == ok
