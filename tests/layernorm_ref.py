"""Float64 reference, exact-data regime, derived error bars and an emulation (with mutations) for the LayerNorm kernels of
csrc/norm_elementwise.hip: mmg_layernorm_fwd, mmg_layernorm_fwd_f32, mmg_layernorm_fwd_fp8, mmg_layernorm_bwd, mmg_layernorm_bwd_f32
(four kernel templates, the 28 instantiations of the kernel table in csrc/layernorm_plan.h, chosen by ln_plan).

Imported by tests/test_layernorm_ref_cpu.py (no GPU: the table names every instantiation and mode, the exactness preconditions hold on
the reference alone, the emulation is inside every bar and every mutation of it leaves them), by tests/test_layernorm_plan_cpu.py (no
GPU: the library's own plans against select / plan below and against the launches recorded before the plan existed) and by
tests/test_layernorm_gpu.py (the kernels against the same reference).  Everything here runs on the CPU.

The operation (xs = the row normalised: x, or fp32(x + res), which the fp32-row forward also writes back over x):
    forward   mean, var = row statistics of xs;  rstd = (var + eps)^-1/2;  xhat = (xs - mean) rstd;  y = xhat gamma + beta
              y is stored as bf16 (plain or 2x2-patchified, the pixels of an odd last row / column dropped), as e4m3 bytes (saturating at
              +-448), and optionally once more as fp32 (yf)
    backward  (mean, rstd are fp32 INPUTS)  xhat = (xs - mean) rstd;  g = dy gamma;  dx = rstd (g - mean(g) - xhat mean(g xhat)) + add
              dgamma += sum_rows dy xhat;  dbeta += sum_rows dy;  a dropped pixel has dy = 0: dx = add (or 0), nothing accumulated

Rows are periodic: row i of a case is row i mod P (P = 257) of a base block, so the reference is computed for at most P rows whatever M
is, equal rows must give equal bits, and the accumulated outputs weigh each base row by its count.

Two data regimes.
  integer   xs rows of +-1 with C/2 of each sign, an independent pattern per row, eps = 3 (mean 0, var 1, rstd 1/2); gamma in {+-2, +-4},
            beta in {-3, 0, 3} (y = +-1, +-2 + beta is never 0: a zero would carry the sign of rstd's last bits); res, add integers in
            [-4, 4] (x = xs - res); dy small integers, adjusted per row so that sum(dy gamma) is a multiple of 2C and sum(dy gamma xhat)
            a multiple of 2C (targets 0, +-2C, varying by row), so the two means of the backward are even integers whether the kernel
            divides by C or multiplies by fp32(1/C).
            EXACT (torch.equal against the reference cast to the output type): mean, x_after, dbeta (integer sums below 2^24 in any
            order, non-zero pre-fill included), every bf16 output (y, patchified y, dx, the dx of dropped pixels) and the e4m3 bytes.
            The module asserts on the reference alone that each of these values sits on the output grid and that the fp32 part of its
            bar is below a quarter ulp of the output type (exactness_violations).
            BARRED with the bf16 terms at zero: rstd (an fp32 rsqrt, and 1/C in the plain kernels), yf, dgamma.
  gaussian  every case of M >= 4 mixes four row flavours: plain; offset by +100; constant (var = 0, y = beta, rstd = eps^-1/2); magnitude
            2^-20.  eps from {1e-6, 1e-12, 1e-5}: 1e-12 with the fp32-row cases (a 2^-20 row has var = 9e-13), 1e-5 at C = 256 / 512.
            fp32 rows are not bf16-exact.

Exact in both regimes: x_after = fp32(x + res); y = bf16(yf); the patchified y is a permutation of the plain y; dx of a dropped pixel.

Bars (u = 2^-24, hulp = half an ulp of the output type at the reference; first order, carried through absolute values).  A group sum
adds 8 CH elements sequentially per lane and then log2 G butterfly steps: no term passes more than D = 8 CH + log2 G additions.
  mean      E_mean = (D + 2) u mean|xs|                                  (the division, or fp32(1/C) and the product)
  rstd      1/2 rstd^3 (2 mean|d| E_mean + E_mean^2 + (D + 6) u (var + eps)) + K_RSQ u rstd,   d = xs - mean
  xhat      E_xhat = rstd (E_mean + 2 u |d|) + |d| E_rstd                                               (not an output)
  y         hulp + E_y,  E_y = |gamma| E_xhat + 2 u (|xhat gamma| + |beta|);   yf: E_y;   fp8: see below
  backward  (mean, rstd given)  E_xh = 2 u |xhat|;  E_g = u |g|;  E_m1 = mean E_g + (D + 2) u mean|g|;
            E_m2 = mean(E_g |xhat| + |g| E_xh) + (D + 3) u mean|g xhat|;  t = g - m1 - xhat m2,
            E_t = E_g + E_m1 + |xhat| E_m2 + |m2| E_xh + 3 u (|g| + |m1| + |xhat m2|)
  dx        hulp + rstd E_t + u |rstd t| + u |dx| [add]
  dgamma    sum_r n_r |dy| E_xh + k u (sum_r n_r |dy xhat| + |F|);   dbeta   k u (sum_r n_r |dy| + |F|);   F = the pre-fill,
            k = min(rows counted, iterations per thread + rows per block + blocks) + 2: each level of the accumulation - a thread's rows,
            the LDS atomics of a block, the global atomics of the grid - is bounded for ANY order of its additions, so no measured factor
            on the atomics is needed (this is never wider than the any-order bound over all rows, (n - 1) u sum|a||b|).
K_RSQ is measured, not derived: the accuracy of the device rsqrtf is not in the code.  See K_RSQ below.

fp8 bytes: a byte may differ from the reference's e4m3 rounding only where the float64 value lies within E_y of a rounding boundary, and
then only to the neighbouring code: the decoded byte must lie in [q(ref - E_y), q(ref + E_y)], q = round-to-nearest-even onto the e4m3
grid.  The share of elements with q(ref - E_y) != q(ref + E_y) is computed from the reference alone and capped at 1 %.

The emulation (emulate) is the kernels' arithmetic in fp32 torch: the lane / chunk dealing (chunk c = lane + k G), the sequential lane
sums and the butterfly, s / C against s fp32(1/C), the rounding points, the patch addressing, the weights of the rows.  MUTATIONS break
one of those at a time."""
import functools
import math
import zlib
from typing import NamedTuple, Optional, Tuple

import torch

BF = torch.bfloat16
F64 = torch.float64
F32 = torch.float32
U32 = 2.0 ** -24
P = 257                        # period of the rows (a prime: no divisor of a block's rows or of a grid)
CAP = {"fwd": 4096, "bwd": 1024}
NT_BYTES = 1 << 28
WIDTHS = (8, 64, 72, 96, 128, 192, 256, 264, 384, 512, 768, 1024, 1032, 1536, 2048, 2056, 3072, 4096)
PLAIN_WIDTHS = (96, 192, 384, 768, 1536)
FILL = {"dgamma": 0.5, "dbeta": -3.0}
# Measured, not derived: the smallest power of two >= 4 x the worst rstd ratio recorded on an MI355X over every gaussian forward case of
# CASES with K_RSQ = 1 (profiles/layernorm_measured_tolerances.jsonl, the records with k_rsq = 1: worst rstd_ratio 0.128 at
# fwd-C8-M73-gaussian, 0.09 - 0.12 at the other widths' plain rows, 0.05 and below on the large cases; 4 x 0.128 = 0.51; DESIGN.md
# "LayerNorm kernels against float64").
K_RSQ = 1.0


def cdiv(a, b):
    return -(-a // b)


class Case(NamedTuple):
    op: str                                    # fwd | bwd
    C: int
    M: int
    regime: str                                # integer | gaussian
    x32: bool = False                          # fp32 rows (mmg_layernorm_fwd_f32 / mmg_layernorm_bwd_f32)
    res: bool = False                          # fwd, x32: x <- x + res first
    yf: bool = False                           # fwd, x32: the fp32 copy of y
    fp8: bool = False                          # fwd: e4m3 output (mmg_layernorm_fwd_fp8)
    patch: Optional[Tuple[int, int]] = None    # (H, W): 2x2-patchified y / dy; M = images x H x W
    add: bool = False                          # bwd
    grads: bool = True                         # bwd: dgamma / dbeta given
    stats: bool = True                         # fwd: mean / rstd given
    strided: str = ""                          # the operand whose leading dimension is wider than its row: x y dy dx add res yf
    pad: int = 8
    plain: Optional[int] = None                # MMG_LN_PLAIN
    ch3: Optional[int] = None                  # MMG_LN_CH3
    eps: float = 1e-6

    @property
    def id(self):
        s = f"{self.op}-C{self.C}-M{self.M}-{self.regime}"
        for tag, on in (("x32", self.x32), ("res", self.res), ("yf", self.yf), ("fp8", self.fp8), ("add", self.add),
                        ("nograds", not self.grads and self.op == "bwd"), ("nostats", not self.stats)):
            if on:
                s += "-" + tag
        if self.patch:
            s += f"-patch{self.patch[0]}x{self.patch[1]}"
        if self.strided:
            s += f"-ld{self.strided}+{self.pad}"
        for tag, v in (("plain", self.plain), ("ch3", self.ch3)):
            if v is not None:
                s += f"-{tag}{v}"
        if self.regime == "gaussian":
            s += f"-eps{self.eps:g}"
        return s

    @property
    def env(self):
        return {"MMG_LN_PLAIN": self.plain, "MMG_LN_CH3": self.ch3}

    @property
    def entry(self):
        if self.op == "fwd":
            return "mmg_layernorm_fwd_fp8" if self.fp8 else "mmg_layernorm_fwd_f32" if self.x32 else "mmg_layernorm_fwd"
        return "mmg_layernorm_bwd_f32" if self.x32 else "mmg_layernorm_bwd"

    @property
    def plan_args(self):
        """The case as mmg_layernorm_plan takes it: (door, M, C, res, yf, add)."""
        return (DOORS.index(self.entry), self.M, self.C, int(self.res), int(self.yf), int(self.add))


DOORS = ("mmg_layernorm_fwd", "mmg_layernorm_fwd_f32", "mmg_layernorm_fwd_fp8", "mmg_layernorm_bwd", "mmg_layernorm_bwd_f32")


# ---- ln_plan's selection (csrc/layernorm_plan.hip), restated: independent of it, never through mmg_layernorm_plan ------------------
def select(case):
    """-> (template: 'plain' | 'generic', G lanes per row, CH chunks per lane)."""
    nch = case.C // 8
    G = 8
    while G < nch and G < 64:
        G <<= 1
    ch = cdiv(nch, G)
    bwd = case.op == "bwd"
    ch3_on = 1 if case.ch3 is None else case.ch3
    plain_on = 1 if case.plain is None else case.plain
    g3 = nch // 3 if nch % 3 == 0 else 0
    ch3 = (not bwd) and bool(ch3_on) and g3 in (8, 16, 32, 64)
    if plain_on and g3 in (4, 8, 16, 32, 64) and not (case.x32 or case.res or case.fp8 or case.yf or case.add):
        return ("plain", g3, 3)
    if ch3:
        return ("generic", g3, 3)
    if G < 64:
        return ("generic", G, 1)
    if ch > 8:
        raise ValueError(f"C={case.C} too wide")
    return ("generic", 64, 1 if ch <= 1 else 2 if ch <= 2 else 4 if ch <= 4 else 8)


def kernel_note(case):
    """mmg_last_kernel() after the case's launch."""
    kind, G, CH = select(case)
    return f"layernorm_{case.op}_plain_kernel<{G}>" if kind == "plain" else f"layernorm_{case.op}_kernel<{G}, {CH}>"


def instantiation(case):
    return (case.op,) + select(case)


def plan(case):
    """dict(rpb rows per block, blocks, iters: rows a thread walks at most, nt: the non-temporal store path)."""
    _, G, _ = select(case)
    rpb = 4 * (64 // G)
    blocks = min(cdiv(case.M, rpb), CAP[case.op])
    return dict(rpb=rpb, rpw=64 // G, blocks=blocks, iters=cdiv(case.M, blocks * rpb), capped=cdiv(case.M, rpb) > CAP[case.op],
                nt=(not case.x32) and (not case.fp8) and case.M * case.C * 2 >= NT_BYTES)


ALL_INSTANTIATIONS = (
    {(op, "plain", G, 3) for op in ("fwd", "bwd") for G in (4, 8, 16, 32, 64)}
    | {("fwd", "generic", G, 3) for G in (8, 16, 32, 64)}
    | {(op, "generic", G, 1) for op in ("fwd", "bwd") for G in (8, 16, 32, 64)}
    | {(op, "generic", 64, CH) for op in ("fwd", "bwd") for CH in (2, 4, 8)})


# ---- the table -------------------------------------------------------------------------------------------------------------------
def ragged(case):
    """Two or three blocks plus a remainder that is no multiple of the rows per wave."""
    pl = plan(case._replace(M=1))
    nb = 2 if (case.C // 8) % 2 else 3
    return case._replace(M=nb * pl["rpb"] + pl["rpw"] + 1)


def _eps(C, x32):
    return 1e-12 if x32 else 1e-5 if C in (256, 512) else 1e-6


def _table():
    T = []

    def both(c, M=None):
        c = ragged(c) if M is None else c._replace(M=M)
        for v in (c._replace(regime="integer"), c._replace(regime="gaussian", eps=_eps(c.C, c.x32))):
            if v not in T:
                T.append(v)

    for C in WIDTHS:                                   # every width, the default selection
        for op in ("fwd", "bwd"):
            both(Case(op, C, 0, ""))
    for C in PLAIN_WIDTHS:                             # the selections behind the two knobs
        both(Case("fwd", C, 0, "", plain=0))
        both(Case("fwd", C, 0, "", plain=0, ch3=0))
        both(Case("fwd", C, 0, "", ch3=0))
        both(Case("bwd", C, 0, "", plain=0))
    both(Case("fwd", 96, 0, ""), M=1)                  # fewer rows than one wave holds
    both(Case("bwd", 96, 0, ""), M=1)
    both(Case("fwd", 384, 0, ""), M=2 * 16)            # whole blocks
    both(Case("bwd", 512, 0, ""), M=3 * 4)
    # every mode at a plain-eligible and at a generic-only width
    for C, pad in ((192, 8), (768, 64), (256, 64), (1032, 8)):
        for res in (False, True):
            for yf in (False, True):
                both(Case("fwd", C, 0, "", x32=True, res=res, yf=yf))
        fp8 = ragged(Case("fwd", C, 0, "", fp8=True))
        both(fp8, M=fp8.M + 128)                       # (128 rows more: the share of offset and constant rows as at large M)
        both(Case("fwd", C, 0, "", stats=False))
        both(Case("fwd", C, 0, "", x32=True, stats=False))
        for add in (False, True):
            for grads in (False, True):
                both(Case("bwd", C, 0, "", add=add, grads=grads))
                both(Case("bwd", C, 0, "", x32=True, add=add, grads=grads))
        for s in ("x", "y"):
            both(Case("fwd", C, 0, "", strided=s, pad=pad))
            both(Case("fwd", C, 0, "", x32=True, res=True, yf=True, strided=s, pad=pad))
        both(fp8._replace(strided="y", pad=pad), M=fp8.M + 128)
        for s in ("res", "yf"):
            both(Case("fwd", C, 0, "", x32=True, res=True, yf=True, strided=s, pad=pad))
        for s in ("x", "dy", "dx"):
            both(Case("bwd", C, 0, "", strided=s, pad=pad))
        both(Case("bwd", C, 0, "", x32=True, strided="x", pad=pad))
        both(Case("bwd", C, 0, "", add=True, strided="add", pad=pad))
    for C in (192, 384, 256, 1024):
        for H, W in ((4, 6), (5, 6), (4, 7), (5, 7)):
            both(Case("fwd", C, 0, "", patch=(H, W)), M=3 * H * W)
            both(Case("bwd", C, 0, "", patch=(H, W)), M=3 * H * W)
            both(Case("bwd", C, 0, "", patch=(H, W), add=True), M=3 * H * W)
        both(Case("fwd", C, 0, "", patch=(5, 7), strided="y"), M=3 * 35)
        both(Case("bwd", C, 0, "", patch=(5, 7), strided="dy", add=True), M=3 * 35)
        both(Case("fwd", C, 0, "", patch=(5, 7), plain=0), M=3 * 35)
    # the grid-stride loop, once per template: cap blocks and a few rows more
    both(Case("fwd", 512, 0, ""), M=4096 * 4 + 5)
    both(Case("fwd", 1536, 0, ""), M=4096 * 4 + 5)
    both(Case("bwd", 512, 0, ""), M=1024 * 4 + 5)
    both(Case("bwd", 96, 0, ""), M=1024 * 64 + 37)
    # the non-temporal stores: M C 2 >= 2^28 bytes
    both(Case("fwd", 1536, 0, ""), M=87381 + 8)
    both(Case("bwd", 1536, 0, ""), M=87381 + 8)
    both(Case("fwd", 1024, 0, ""), M=131072 + 5)
    both(Case("bwd", 1024, 0, ""), M=131072 + 5)
    return T


CASES = _table()


# ---- patch addressing ------------------------------------------------------------------------------------------------------------
def patch_map(M, H, W, swap=False, wrule=False):
    """ln_out_offset for rows 0 .. M-1 -> (live mask, patch row, quadrant).  swap / wrule: two of the MUTATIONS."""
    m = torch.arange(M)
    w, h, n = m % W, (m // W) % H, m // (W * H)
    live = (h < (H & ~1)) & (w < (W if wrule else W & ~1))
    prow = (n * (H // 2) + (h >> 1)) * (W // 2) + (w >> 1)
    quad = (w & 1) * 2 + (h & 1) if swap else (h & 1) * 2 + (w & 1)
    return live, prow, quad


def patch_rows(M, H, W):
    return (M // (H * W)) * (H // 2) * (W // 2)


def to_patch(rows, H, W):
    """[M, C] rows -> the [patch_rows, 4C] matrix the forward writes (dropped pixels have no place in it)."""
    M, C = rows.shape
    live, prow, quad = patch_map(M, H, W)
    out = torch.zeros(patch_rows(M, H, W), 4, C, dtype=rows.dtype, device=rows.device)
    out[prow[live].to(rows.device), quad[live].to(rows.device)] = rows[live.to(rows.device)]
    return out.reshape(-1, 4 * C)


def from_patch(mat, M, H, W):
    """The inverse: [patch_rows, >= 4C] -> [M, C]; the rows of dropped pixels are zero."""
    C = mat.shape[1] // 4
    live, prow, quad = patch_map(M, H, W)
    dev = mat.device
    v = mat[:, :4 * C].reshape(-1, 4, C)
    out = torch.zeros(M, C, dtype=mat.dtype, device=dev)
    out[live.to(dev)] = v[prow[live].to(dev), quad[live].to(dev)]
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _rb(x):
    return x.to(F32).to(BF).to(F64)


def _r32(x):
    return x.to(F32).to(F64)


def half_ulp_bf16(v):
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 9)


def q8(v):
    """Round to nearest even onto the e4m3 grid, saturating at +-448 (float64 in, float64 out)."""
    v = v.clamp(-448.0, 448.0)
    _, ex = torch.frexp(v.abs().clamp_min(2.0 ** -20))
    step = torch.ldexp(torch.ones_like(v), (ex - 1).clamp_min(-6) - 3)
    return torch.round(v / step) * step


def base_rows(case):
    return min(case.M, P)


def data_key(case):
    return (case.C, case.regime, base_rows(case), case.x32, case.res, case.eps if case.regime == "gaussian" else 3.0, case.fp8)


def make_data(case):
    """dict of float64 tensors for the base block: x (as stored: bf16-exact, or fp32-exact with x32), res, xs (the row normalised),
    gamma, beta, dy, add (bf16-exact), eps, mean32 / rstd32 (the backward's inputs: the reference statistics rounded to fp32)."""
    C, regime, n, x32, has_res, eps, fp8 = data_key(case)
    g = torch.Generator().manual_seed(zlib.crc32(repr(data_key(case)).encode()))
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=F64)
    d = {}
    if regime == "integer":
        gamma = (ri(0, 1, C) * 2 + 2) * (ri(0, 1, C) * 2 - 1)
        two = gamma.abs() == 2
        if int(two.sum()) < 2:
            gamma[:2] = torch.tensor([2.0, -2.0], dtype=F64)
            two = gamma.abs() == 2
        xs = torch.ones(n, C, dtype=F64)
        for r in range(n):
            while True:                                    # C/2 of each sign, and a |gamma| = 2 column of each sign of x
                row = torch.ones(C, dtype=F64)
                row[torch.randperm(C, generator=g)[:C // 2]] = -1.0
                if bool((two & (row > 0)).any()) and bool((two & (row < 0)).any()):
                    break
            xs[r] = row
        dy = ri(-2, 2, n, C)
        gg = dy * gamma
        a, b = gg.sum(1), (gg * xs).sum(1)                  # sum g, sum g x = 2 sum g xhat
        ta = (torch.arange(n) % 3 - 1).to(F64) * 2 * C      # targets: 0, +-2C;  0, +-4C for sum g x
        tb = ((torch.arange(n) // 3) % 3 - 1).to(F64) * 4 * C
        dp, dn = (ta - a + tb - b) / 4, (ta - a - tb + b) / 4
        sg = torch.sign(gamma)
        for r in range(n):
            for cols, delta in ((two & (xs[r] > 0), dp[r]), (two & (xs[r] < 0), dn[r])):
                idx = cols.nonzero().flatten()
                k = len(idx)
                q, rem = divmod(int(abs(delta)), k)
                inc = torch.full((k,), float(q), dtype=F64)
                inc[:rem] += 1
                dy[r, idx] += math.copysign(1.0, float(delta)) * inc * sg[idx]
        res = ri(-4, 4, n, C) if has_res else None
        d.update(xs=xs, x=xs - res if has_res else xs, res=res, gamma=gamma, beta=ri(-1, 1, C) * 3, dy=dy, add=ri(-4, 4, n, C), eps=3.0)
    else:
        rnd = _r32 if x32 else _rb
        z = rn(n, C)
        res = _r32(rn(n, C)) if has_res else None
        const = torch.zeros(n, dtype=torch.bool)
        if n >= 4:
            for r in range(n):
                if r % 8 == 1:
                    z[r] += 100.0
                elif r % 64 == 2:
                    # (a few bits: every partial sum of the row is exact.  fp8: 2^-6 of it, so that the row's bar, rstd E_mean =
                    #  2e-3 |value| at eps = 1e-6, stays well inside an e4m3 step at beta - the boundary share is capped at 1 %)
                    z[r] = torch.round(z[r, 0] * 1024) / 1024 * (2.0 ** -6 if fp8 else 1.0)
                    const[r] = True
                elif r % 64 == 3:
                    z[r] *= 2.0 ** -20
        if has_res:
            res[const] = torch.round(res[const] * 1024) / 1024       # x + res is exact there: the row stays constant
            x = rnd(z - res)
            xs = _r32(x + res)
        else:
            x = xs = rnd(z)
        d.update(xs=xs, x=x, res=res, gamma=_r32(1 + 0.2 * rn(C)), beta=_r32(0.1 * rn(C)), dy=_rb(0.5 * rn(n, C)), add=_rb(rn(n, C)),
                 eps=float(torch.tensor(eps, dtype=F32)))
    mean = d["xs"].mean(1)
    dv = d["xs"] - mean[:, None]
    d["mean32"], d["rstd32"] = _r32(mean), _r32(((dv * dv).mean(1) + d["eps"]) ** -0.5)
    return d


def counts(M, n):
    return torch.bincount(torch.arange(M) % n, minlength=n).to(F64)


def live_rows(case):
    """Mask over the base rows: the pixels a patchified case keeps (everything otherwise)."""
    n = base_rows(case)
    if not case.patch:
        return torch.ones(n, dtype=torch.bool)
    assert case.M <= P and case.M % (case.patch[0] * case.patch[1]) == 0
    return patch_map(case.M, *case.patch)[0]


def outputs_of(case):
    if case.op == "fwd":
        return ("y",) + (("mean", "rstd") if case.stats else ()) + (("yf",) if case.yf else ()) + (("x_after",) if case.res else ())
    return ("dx",) + (("dgamma", "dbeta") if case.grads else ())


def exact_outputs(case):
    """Outputs compared with torch.equal."""
    if case.regime != "integer":
        return ("x_after",)
    return ("y", "mean", "x_after", "dx", "dbeta")


# ---- reference and bars ----------------------------------------------------------------------------------------------------------
def reference(case, d):
    """-> (ref, bar, ebar): float64 per base row ([n, C] in the row layout also for patchified cases; rows of dropped pixels: y is
    not written - the tests skip them -, dx = add or 0 with a zero bar) or per column (dgamma, dbeta: the whole launch of M rows).
    ebar: the bars without their hulp term (the fp32 part)."""
    integer = case.regime == "integer"
    A = torch.abs
    u = U32
    C = case.C
    _, G, CH = select(case)
    D = 8 * CH + int(math.log2(G))
    xs, gamma, beta, eps = d["xs"], d["gamma"], d["beta"], d["eps"]
    live = live_rows(case)
    hu = (lambda t: torch.zeros_like(t)) if integer else half_ulp_bf16
    if case.op == "fwd":
        mean = xs.mean(1)
        dv = xs - mean[:, None]
        var = (dv * dv).mean(1)
        rstd = (var + eps) ** -0.5
        xhat = dv * rstd[:, None]
        y = xhat * gamma + beta
        e_mean = (D + 2) * u * A(xs).mean(1)
        e_rstd = 0.5 * rstd ** 3 * (2 * A(dv).mean(1) * e_mean + e_mean ** 2 + (D + 6) * u * (var + eps)) + K_RSQ * u * rstd
        e_xhat = rstd[:, None] * (e_mean[:, None] + 2 * u * A(dv)) + A(dv) * e_rstd[:, None]
        e_y = A(gamma) * e_xhat + 2 * u * (A(xhat * gamma) + A(beta))
        lv = live[:, None].to(F64)                             # a dropped pixel has no y: zero here, as from_patch gives it
        ref = dict(mean=mean, rstd=rstd, y=y * lv, yf=y, x_after=xs)
        ebar = dict(mean=e_mean, rstd=e_rstd, y=e_y * lv, yf=e_y, x_after=torch.zeros_like(xs))
        bar = dict(ebar, y=(e_y + (0 if case.fp8 else hu(y))) * lv)
        return ref, bar, ebar
    mu, rs = d["mean32"][:, None], d["rstd32"][:, None]
    dy = d["dy"] * live[:, None].to(F64)
    add = d["add"] if case.add else torch.zeros_like(xs)
    xh = (xs - mu) * rs
    g = dy * gamma
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    t = g - m1 - xh * m2
    dx = rs * t + add
    e_xh, e_g = 2 * u * A(xh), u * A(g)
    e_m1 = e_g.mean(1, keepdim=True) + (D + 2) * u * A(g).mean(1, keepdim=True)
    e_m2 = (e_g * A(xh) + A(g) * e_xh).mean(1, keepdim=True) + (D + 3) * u * A(g * xh).mean(1, keepdim=True)
    e_t = e_g + e_m1 + A(xh) * e_m2 + A(m2) * e_xh + 3 * u * (A(g) + A(m1) + A(xh * m2))
    e_dx = rs * e_t + u * A(rs * t) + (u * A(dx) if case.add else 0.0)
    e_dx = e_dx * live[:, None].to(F64)                    # a dropped pixel: dx = add (or 0) exactly
    n = xs.shape[0]
    w = (counts(case.M, n) * live.to(F64))[:, None]
    pl = plan(case)
    k = min(float(w.sum()), pl["iters"] + pl["rpb"] + pl["blocks"]) + 2
    ref = dict(dx=dx, dgamma=(w * dy * xh).sum(0) + FILL["dgamma"], dbeta=(w * dy).sum(0) + FILL["dbeta"])
    ebar = dict(dx=e_dx, dgamma=(w * A(dy) * e_xh).sum(0) + k * u * ((w * A(dy * xh)).sum(0) + abs(FILL["dgamma"])),
                dbeta=k * u * ((w * A(dy)).sum(0) + abs(FILL["dbeta"])))
    bar = dict(ebar, dx=e_dx + hu(dx) * live[:, None].to(F64))
    return ref, bar, ebar


@functools.lru_cache(maxsize=8)
def _prepared(case):
    d = make_data(case)
    return (d,) + reference(case, d)


def prepared(case):
    """(data, ref, bar, ebar) of a case, shared: callers must not modify them."""
    return _prepared(case._replace(strided="", pad=8))


def fp8_boundary_share(ref_y, e_y):
    return (q8(ref_y - e_y) != q8(ref_y + e_y)).double().mean().item()


def exactness_violations(case, d, ref, ebar):
    """Why torch.equal would NOT be justified for this integer case (empty list: it is)."""
    bad = []
    A = torch.abs
    xs = d["xs"]
    if not (bool((A(xs) == 1).all()) and bool((xs.sum(1) == 0).all()) and d["eps"] == 3.0):
        bad.append("rows are not +-1 with C/2 of each sign at eps = 3")
    if len({tuple(r.tolist()) for r in xs[:8]}) <= min(8, xs.shape[0]) // 2:       # (C = 8 has 70 patterns: a repeat can happen)
        bad.append("the sign pattern does not differ from row to row")
    if not set(A(d["gamma"]).tolist()) <= {2.0, 4.0}:
        bad.append("gamma is not in {+-2, +-4}")
    if case.op == "fwd":
        if not (torch.equal(ref["mean"], torch.zeros_like(ref["mean"])) and torch.equal(ref["rstd"], torch.full_like(ref["rstd"], 0.5))):
            bad.append("mean is not 0 / rstd is not 1/2")
        y = ref["y"][live_rows(case)]
        ey = ebar["y"][live_rows(case)]
        grid, quarter = (q8(y), 0.25 * 2.0 ** -3 * A(y) / 2) if case.fp8 else (_rb(y), 0.5 * half_ulp_bf16(y))
        if not torch.equal(grid, y) or bool((y == 0).any()):
            bad.append("y is off the output grid, or zero")
        if not bool((ey < quarter).all()):
            bad.append("the fp32 error of y could reach a quarter ulp of the output type")
        if case.res and not torch.equal(_r32(d["x"] + d["res"]), d["x"] + d["res"]):
            bad.append("x + res is not exact")
        return bad
    C = case.C
    g = d["dy"] * d["gamma"]
    s1, s2 = g.sum(1), (g * xs * 0.5).sum(1)
    if not (bool((s1 % (2 * C) == 0).all()) and bool((s2 % (2 * C) == 0).all())):
        bad.append("sum(dy gamma) or sum(dy gamma xhat) is not a multiple of 2C")
    if not (bool((s1 != 0).any()) and bool((s2 != 0).any())) and xs.shape[0] >= 9:
        bad.append("both means of the backward are zero in every row")
    if not torch.equal(_rb(ref["dx"]), ref["dx"]):
        bad.append("dx is off the bf16 grid")
    w = counts(case.M, xs.shape[0])[:, None]
    if float((w * A(d["dy"])).sum(0).max()) + 3 >= 2 ** 24 or float(A(g).sum(1).max()) >= 2 ** 23:
        bad.append("a partial sum could pass 2^24")
    if not torch.equal(ref["dbeta"], ref["dbeta"].round()):
        bad.append("dbeta is not an integer")
    return bad


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def check(case, name, got, ref, bar):
    """got against ref (float64, same shape) -> (worst ratio to the bar, share of elements that differ from the reference cast to the
    output type).  Exact outputs: the ratio is 0.0 (equal) or inf.  A zero bar demands equality."""
    fp8 = name == "y" and case.fp8
    cast = q8(ref) if fp8 else _rb(ref) if name in ("y", "dx") else _r32(ref)
    differ = (got != cast).double().mean().item()
    if not torch.isfinite(got).all():
        return float("inf"), differ
    if name in exact_outputs(case):
        return (0.0 if differ == 0 else float("inf")), differ
    if fp8:
        inside = (got >= q8(ref - bar)) & (got <= q8(ref + bar))
        return (0.0 if bool(inside.all()) else float("inf")), differ
    diff = (got - ref).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bar)
    return ratio.max().item(), differ


# ---- emulation of the launch, and mutations of it --------------------------------------------------------------------------------
MUTATIONS = ("eps_dropped", "eps_after_sqrt", "var_over_c_minus_1", "lane_dropped", "chunk_dropped", "gamma_chunk_off_by_G",
             "s2_not_divided", "dgamma_from_g", "dbeta_plus_beta", "dropped_pixel_counted", "row_past_M_counted", "add_dropped",
             "res_not_written", "yf_after_bf16", "quadrant_swapped", "w_rule", "neighbour_stats")


def mutation_applies(case, mut):
    """Whether the case contains the feature a mutation breaks."""
    fwd, bwd = case.op == "fwd", case.op == "bwd"
    _, G, CH = select(case)
    nch = case.C // 8
    gauss = case.regime == "gaussian"
    return {
        "eps_dropped": fwd and (not gauss or base_rows(case) >= 4),          # (gaussian: the constant row)
        "eps_after_sqrt": fwd and (not gauss or base_rows(case) >= 4),
        "var_over_c_minus_1": fwd and (gauss or case.stats),    # (integer: eps = 3 leaves 1/8C of it, which y's rounding hides)
        "lane_dropped": nch >= G and (fwd or bwd), "chunk_dropped": True,
        "gamma_chunk_off_by_G": nch > G,
        "s2_not_divided": bwd, "dgamma_from_g": bwd and case.grads, "dbeta_plus_beta": bwd and case.grads,
        "dropped_pixel_counted": bwd and case.grads and bool(case.patch) and (case.patch[0] % 2 or case.patch[1] % 2) == 1,
        # (gaussian: one row among M must exceed k u sum|dy|; the integer dbeta is exact at any M)
        "row_past_M_counted": bwd and case.grads and not case.patch and (not gauss or case.M <= 5000),
        "add_dropped": bwd and case.add, "res_not_written": fwd and case.res, "yf_after_bf16": fwd and case.yf and gauss,
        "quadrant_swapped": bool(case.patch), "w_rule": bool(case.patch) and case.patch[1] % 2 == 1,
        "neighbour_stats": gauss and base_rows(case) >= 4 and (bwd or case.stats),
    }[mut]


def _f(t):
    return t.to(F32)


def _group_sum(v, G, CH, mut):
    """v [n, C] fp32 -> [n] fp32: 8 elements x CH chunks sequentially per lane (chunk c = lane + k G), then the butterfly."""
    n, C = v.shape
    nch = C // 8
    pad = torch.zeros(n, G * CH, 8, dtype=F32)
    pad[:, :nch] = v.reshape(n, nch, 8)
    if mut == "chunk_dropped":
        pad[:, nch - 1] = 0
    lanes = pad.reshape(n, CH, G, 8)
    s = torch.zeros(n, G, dtype=F32)
    for k in range(CH):
        for e in range(8):
            s = s + lanes[:, k, :, e]
    if mut == "lane_dropped":
        s[:, G - 1] = 0
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def emulate(case, d, mut=None):
    """The launch on the base rows -> {output: float64} in the row layout (patchified y: as from_patch gives it; rows of dropped
    pixels zero); accumulated outputs for all M rows.  mut: one of MUTATIONS."""
    kind, G, CH = select(case)
    C, M = case.C, case.M
    n = base_rows(case)
    nch = C // 8
    plain = kind == "plain"
    inv_c = torch.tensor(1.0, dtype=F32) / torch.tensor(float(C), dtype=F32)
    over_c = (lambda s: s * inv_c) if plain else (lambda s: s / torch.tensor(float(C), dtype=F32))
    gamma, beta = _f(d["gamma"]), _f(d["beta"])
    if mut == "gamma_chunk_off_by_G":
        gamma = gamma.reshape(nch, 8).roll(-G, 0).reshape(-1)
    eps = torch.tensor(d["eps"], dtype=F32)
    x = _f(d["x"])
    if case.op == "fwd":
        xs = x + _f(d["res"]) if case.res else x
        mu = over_c(_group_sum(xs, G, CH, mut))
        dv = xs - mu[:, None]
        q = _group_sum(dv * dv, G, CH, mut)
        var = q / torch.tensor(float(C - 1), dtype=F32) if mut == "var_over_c_minus_1" else over_c(q)
        if mut == "eps_after_sqrt":
            rs = 1.0 / (torch.sqrt(var) + eps)
        else:
            rs = torch.rsqrt(var + (0.0 if mut == "eps_dropped" else eps))
        o = dv * rs[:, None] * gamma + beta
        if case.fp8:
            y = q8(o.to(F64))
        else:
            y = o.to(BF).to(F64)
        if case.patch:
            H, W = case.patch
            live, prow, quad = patch_map(M, H, W, swap=mut == "quadrant_swapped", wrule=mut == "w_rule")
            buf = torch.full((patch_rows(M, H, W) + W, 4, C), float("nan"), dtype=F64)        # (+ W: where w_rule writes past the end)
            true_live = patch_map(M, H, W)[0]
            for sel in (live & true_live, live & ~true_live):                                 # (what w_rule adds is written last)
                buf[prow[sel], quad[sel]] = y[sel]
            y = from_patch(buf[:patch_rows(M, H, W)].reshape(-1, 4 * C), M, H, W)
        out = dict(y=y, yf=(o.to(BF) if mut == "yf_after_bf16" else o).to(F64), mean=mu.to(F64), rstd=rs.to(F64),
                   x_after=(x if mut == "res_not_written" else xs).to(F64))
        if mut == "neighbour_stats":
            out["mean"], out["rstd"] = out["mean"].roll(-1), out["rstd"].roll(-1)
        return {k: out[k] for k in outputs_of(case)}
    mu, rs = _f(d["mean32"]), _f(d["rstd32"])
    if mut == "neighbour_stats":
        mu, rs = mu.roll(-1), rs.roll(-1)
    dy = _f(d["dy"])
    live = live_rows(case)
    counted = live.clone()
    if case.patch:
        H, W = case.patch
        mat = to_patch(dy, H, W)
        mlive, prow, quad = patch_map(M, H, W, swap=mut == "quadrant_swapped", wrule=mut == "w_rule")
        ok = mlive & (prow < mat.shape[0])
        rows_ = torch.zeros_like(dy)
        rows_[ok] = mat.reshape(-1, 4, C)[prow[ok], quad[ok]]
        if mut == "dropped_pixel_counted":                 # the clamped load (offset 0: pixel 0's dy) without the zero select
            rows_[~mlive] = dy[0]
            counted = torch.ones_like(live)
        dy = rows_
    xh = (x - mu[:, None]) * rs[:, None]
    g = dy * gamma
    s1 = over_c(_group_sum(g, G, CH, mut))
    s2 = _group_sum(g * xh, G, CH, mut)
    if mut != "s2_not_divided":
        s2 = over_c(s2)
    if plain:
        o = rs[:, None] * (g - s1[:, None] - (x - mu[:, None]) * rs[:, None] * s2[:, None])
    else:
        o = rs[:, None] * (g - s1[:, None] - xh * s2[:, None])
    if case.add and mut != "add_dropped":
        o = o + _f(d["add"])
    out = dict(dx=o.to(BF).to(F64))
    if case.grads:
        w = counts(M, n) * counted.to(F64)
        if mut == "row_past_M_counted":
            w[M % n] += 1
        w = w[:, None]
        a = (g if mut == "dgamma_from_g" else dy) * xh
        b = dy + beta if mut == "dbeta_plus_beta" else dy
        out["dgamma"] = _r32((w * a.to(F64)).sum(0) + FILL["dgamma"])
        out["dbeta"] = _r32((w * b.to(F64)).sum(0) + FILL["dbeta"])
    return out
