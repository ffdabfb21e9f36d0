"""Float64 reference, exact-data regime, derived error bars and an emulation (with mutations) for the fused ConvNeXt block MLP kernels
of csrc/cnblock_mlp.hip (mmg_cnblock_mlp_fwd, mmg_cnblock_mlp_bwd) and csrc/cnblock_bwdw.hip (mmg_cnblock_bwdw, two launches).

Imported by tests/test_cnblock_ref_cpu.py (no GPU: the table names every template instantiation, the exactness preconditions hold on
the reference alone, the emulation is inside every bar and every mutation of it leaves them) and by tests/test_cnblock_gpu.py (the
kernels against the same reference); tests/test_cnblock_plan_cpu.py holds the library's plans (mmg_cnblock_plan) against the restatement
of the launch rules below.  Everything here runs on the CPU in float64.

The operation (x = xd [M, C], W1 [4C, C], W2 [C, 4C], ls = layer scale [C]; W1, W2 are given bf16-exact - the kernels' contract):
    mean, rstd = row statistics of x, rstd = (var + eps)^-1/2;  xhat = (x - mean) rstd;  xln = xhat ln_w + ln_b
    h = xln W1^T + b1;  g = GELU(h);  y = residual + ls (g W2^T + b2)                                          forward
    dG = dy W2g, W2g = bf16(ls W2);  dh = dG GELU'(h);  dxln = dh W1                                          mlp_bwd (C = 384: h is the
    with ln_grads: dd = rstd (q - mean(q) - xhat mean(q xhat)), q = dxln ln_w;  ln_dw += sum dxln xhat;  ln_db += sum dxln      saved hpre)
    bwdw: h = xhat W1g^T + b1f with W1g = bf16(W1 ln_w), b1f = b1 + W1 ln_b;  dW2raw += dy^T g;  db2raw += sum dy;  db1 += sum dh;
          dW1 += ln_w (dh^T xhat) + db1 ln_b^T;  dln = dh W1;  ln_db += sum dln;  ln_dw += sum dln xhat;  dd as above with q = dln ln_w

Rows are periodic: row i of a case is row i mod P (P = 257) of a base block, so the reference is computed for at most P rows whatever M
is, equal rows must give equal bits, and the accumulated outputs weigh each base row by its count.

Two data regimes.
  integer   rows of +-1 with C/2 of each sign and eps = 3 (mean 0, var 1, rstd 1/2), ln_w in {+-2, +-4}, small integers elsewhere, the
            layer scale a power of two, |h| >= 8 (GELU is x or 0, GELU' 1 or 0 beyond the +-4 clamp; mlp_bwd: h >= 8 only, its GELU' is
            1.0005 there and bf16(dG 1.0005) = bf16(dG) is asserted).  Every fp32 partial sum is an integer or a multiple of 1/2 below
            2^24 in any order and every bf16 rounding is of an exactly known value.
            EXACT (torch.equal against the reference cast to the output type): y, hpre (both kinds), xln, gact; g, dh, dxln without
            ln_grads; db2raw, dW2raw, db1, dW1, ln_db (both kernels), b1f, mean (= 0 x 1/C), and the ln_dw of cnblock_bwdw (its xhat is
            the bf16 image, exactly +-1/2).
            BARRED (an fp32 rstd = rsqrt(4) of unknown last bits, or an fp32 1/C, intervenes; the bar below with its bf16 terms at
            zero): rstd; dd of both kernels; ln_dw of mlp_bwd (fp32 xhat = x rstd).
  gaussian  eps = 1e-6; rows in four flavours in every case of M >= 4: plain, offset by +100, constant (var = 0, xhat = 0, rstd =
            eps^-1/2) and of magnitude 2^-20.  The only regime where the bf16 terms of the bars are live.

Bars (gaussian; u = 2^-24, hulp = half a bf16 ulp of the reference, E_* = first-order error bounds carried through absolute values;
a bf16 rounding point contributes 2^-8 |value|: 2^-9 for the rounding, 2^-9 spare).  Kd(n) = 2 n + 16 fp32 roundings for a dot
product of n terms on the matrix cores (whose adder is not documented to round to nearest: one ulp = 2 u per step).
  mean      K_ACC u mean|x|
  rstd      1/2 rstd^3 (2 mean|d| E_mean + E_mean^2 + K_ACC u (var + eps)) + K_ACC u rstd
  xhat      E_xhat = rstd (E_mean + 2 u |d|) + |d| E_rstd                                              (not an output)
  xln       hulp + |ln_w| E_xhat + 2 u (|xhat ln_w| + |ln_b|)
  h / hpre  hulp + E_h,  E_h = (2^-8 |xln| + E_xln) |W1|^T + Kd(C) u (|xln| |W1|^T + |b1|)   (mlp_bwd at 384: E_h = 2^-8 |h|, the saved hpre;
            bwdw: xhat, W1g, b1f in the place of xln, W1, b1, plus E_b1f = Kd(C) u (|b1| + |W1| |ln_b|), which is also the bar of b1f)
  g / gact  hulp + E_g,  E_g = 1.13 E_h + 5.8e-4 (|g| + 1.13 E_h) + 2.4e-4 [h < E_h] + u |g|          (1.13 >= max |GELU'|)
  hpre kind 1   hulp + 0.8 E_h + 5.5e-4                                                           (0.8 >= max |GELU''|)
  y         hulp + |ls| (E_acc + u (|acc| + |b2|)) + 2 u (|res| + |ls (acc + b2)|),  E_acc = (2^-8 |g| + E_g) |W2|^T + Kd(4C) u |g| |W2|^T
  dh        hulp + E_dh,  E_dh = |dG| E_dg + E_dG (|GELU'| + E_dg) + u |dh|,  E_dG = Kd(C) u |dy| |W2g|,  E_dg = 0.8 E_h + 5.5e-4
  dxln      hulp + E_dx,  E_dx = (2^-8 |dh| + E_dh) |W1| + Kd(4C) u |dh| |W1|     (bwdw: the same product from the dh LDS image - the same
            bits as the bf16 dh operand of dW1, so one rounding point, not two)
  dd        hulp + rstd E_t + E_rstd |t| + u |dd|,  t = q - m1 - xhat m2,  E_t = E_q + E_m1 + |xhat| E_m2 + |m2| E_x + 3 u (|q| + |m1| + |xhat m2|)
            with E_q = |ln_w| E_dx + u |q|, E_m1 = mean E_q + Kd(C) u mean|q|, E_m2 = mean(E_q |xhat| + |q| E_x) + Kd(C) u mean|q xhat|,
            E_x = E_xhat (mlp_bwd, fp32 xhat) or 2^-8 |xhat| + E_xhat (bwdw, bf16 image)
  accumulated (fp32 atomics; rows weighed by their count n_r, F = the pre-fill):   sum_r n_r (operand terms) + K_ACC u (sum_r n_r |a||b| + |F|)
            ln_db: a = dxln, b = 1;  ln_dw: a = dxln, b = xhat;  db2raw: dy;  dW2raw: dy, g;  db1: dh;  dW1: ln_w (dh, xhat) + ln_b db1
K_ACC is measured, not derived (the order of the lanes, shuffles, LDS reductions and atomics is unknown): see K_ACC below.

The emulation (emulate) is the same arithmetic with the kernels' rounding points switched on, the polynomial GELU forms of
csrc/common.h, the weights taken through the packed images (hidden unit 8q + 4tt + r at row position 16 tt + 4q + r of a 32-unit group,
the output columns by the same rule), chunk by chunk, and the rows dealt to workgroup (wave) tiles as the launchers do, rows >= M read
from row M - 1 and never stored.  MUTATIONS break one of those at a time."""
import functools
import math
import zlib
from typing import NamedTuple, Optional

import torch

BF = torch.bfloat16
F64 = torch.float64
U32 = 2.0 ** -24
U8 = 2.0 ** -8
P = 257                  # period of the rows (a prime: no divisor of a tile or of a grid)
BM = 128                 # rows per workgroup tile of cnblock_mlp (every width: 4 waves x 32 rows or 8 waves x 16)
BW_R = 64                # rows per tile of cnblock_bwdw
WIDTHS = (96, 128, 192, 256, 384, 512)
BWD_WIDTHS = (96, 128, 192, 384)
# Measured, not derived: the smallest power of two >= 4 x the worst ratio recorded on an MI355X over every gaussian case of CASES with
# K_ACC = 1 (profiles/cnblock_measured_tolerances.jsonl, the records with k_acc = 1: db2raw 3.31 at 32 832 rows - column sums of dy
# through bf16 fragments, lanes, shuffles and the atomics of 256 workgroups -, rstd 1.47, mean 0.85, every other accumulated output
# below 0.07; 4 x 3.31 = 13.3; DESIGN.md "Fused CNBlock MLP kernels against float64").  The CPU file shows that a bar this wide still
# catches one tail row counted into ln_dw / ln_db and a dW1 without its db1 ln_b^T term.
K_ACC = 16.0
FILL = {"ln_dw": 0.5, "ln_db": -0.25, "dW1": 0.25, "db1": -1.0, "dW2raw": 0.5, "db2raw": 2.0}     # the accumulators' pre-fill
GELU_REL, GELU_NEG, GELUP_ABS = 5.8e-4, 2.4e-4, 5.5e-4          # the documented bars of the polynomial forms (csrc/common.h)
LIP1, LIP2 = 1.13, 0.8                                          # >= max |GELU'| (1.129), >= max |GELU''| (0.798)


def kd(n):
    return 2.0 * n + 16.0


def cdiv(a, b):
    return -(-a // b)


class Case(NamedTuple):
    op: str                        # fwd | bwd | bwdw
    C: int
    M: int                         # rows; 0 = the tile-loop case: rows(case, cus)
    regime: str                    # integer | gaussian
    save: int = 0                  # fwd: 0 nothing, 1 hpre + stats, 2 + xln, 3 + xln + gact, 4 = 3 with hpre_kind 1
    res: Optional[int] = None      # MMG_MLP_FWD_RES (C = 96)
    nt: Optional[int] = None       # MMG_MLP_NT_STORE
    ln: bool = False               # bwd: ln_grads given
    var: Optional[int] = None      # MMG_BWDW_VAR
    hto: Optional[int] = None      # MMG_BWDW_HTO
    w12: Optional[int] = None      # MMG_BWDW_W12

    @property
    def id(self):
        s = f"{self.op}-C{self.C}-M{self.M or 'loop'}-{self.regime}"
        if self.op == "fwd":
            s += f"-save{self.save}"
        if self.ln:
            s += "-ln"
        for tag, v in (("res", self.res), ("nt", self.nt), ("var", self.var), ("hto", self.hto), ("w12", self.w12)):
            if v is not None:
                s += f"-{tag}{v}"
        return s

    @property
    def env(self):
        """The five knobs: {name: value or None (unset)}."""
        return {"MMG_MLP_FWD_RES": self.res, "MMG_MLP_NT_STORE": self.nt, "MMG_BWDW_VAR": self.var, "MMG_BWDW_HTO": self.hto,
                "MMG_BWDW_W12": self.w12}

    @property
    def loop(self):
        return self.M == 0


# ---- the launchers' arithmetic, restated -----------------------------------------------------------------------------------------
def mt(C):
    return 2 if C <= 256 else 1


def resident(case):
    """Waves per workgroup of the resident forward (C = 96, nothing saved, MMG_MLP_FWD_RES 8 / 12; unset = 12), or 0."""
    if case.op != "fwd" or case.C != 96 or case.save:
        return 0
    rw = 12 if case.res is None else case.res
    return rw if rw in (8, 12) else 0


def cap(case, cus):
    """The launcher's grid limit, in workgroups."""
    if case.op == "bwdw":
        return cus
    if case.op == "bwd":
        return (2 if case.C <= 192 else 1) * cus
    if resident(case):
        return cus
    return (3 if case.C <= 96 else 2 if case.C <= 192 else 1) * cus


def rows(case, cus):
    """M of a case: the tile-loop cases run 2 cap + 1 tiles (+ 5 rows where the kernel takes tails)."""
    if not case.loop:
        return case.M
    if case.op == "bwdw":
        return BW_R * (2 * cap(case, cus) + 1)
    rw = resident(case)
    if rw:
        return 32 * (2 * rw * cap(case, cus) + 1) + 5
    return BM * (2 * cap(case, cus) + 1) + 5


def plan(case, cus):
    """dict(M, tile (rows per walked tile), ntiles, walkers (workgroups, or waves of the resident form), min_tiles per walker)."""
    M = rows(case, cus)
    rw = resident(case)
    tile = BW_R if case.op == "bwdw" else 32 if rw else BM
    ntiles = cdiv(M, tile)
    grid = min(cdiv(ntiles, rw), cus) if rw else min(ntiles, cap(case, cus))
    walkers = grid * (rw or 1)
    return dict(M=M, tile=tile, ntiles=ntiles, grid=grid, walkers=walkers, min_tiles=ntiles // walkers, max_tiles=cdiv(ntiles, walkers))


def block(case):
    """Threads per workgroup (cnblock_bwdw: of launch 1 and of launch 2)."""
    if case.op == "bwdw":
        return (768 if case.w12 else 512, 512)
    rw = resident(case)
    return 64 * (rw or (4 if case.C <= 256 else 8))


def lds(case):
    """Dynamic LDS bytes of the launch."""
    C = case.C
    if case.op == "bwdw":
        # the W1 image and the dh image at a hidden pitch of 4C + 8, two row images at a pitch of 64 + 8 rows, ln_w, b1', the row statistics
        return (C // 8) * (4 * C + 8) * 16 + 2 * (C // 8) * 72 * 16 + 4 * 4 * (4 * C + 8) * 8 + C * 4 + 4 * C * 4 + 2 * 64 * 2 * 4
    NC = 64 if C <= 128 else 32
    part = NC * C * 2                                   # one weight part of a chunk, bf16
    if case.op == "bwd":
        return 2 * ((3 if C != 384 else 2) * part) + 8 * C * 4
    return (4 * C // NC if resident(case) else 2) * (2 * part) + 8 * C * 4


def nt(case, M):
    """Whether the 4C-wide outputs are stored past L2: the knob where it is set, else the backward from C = 128 at 256 MiB; a forward
    that saves nothing has no such output."""
    if case.op == "bwdw" or (case.op == "fwd" and not case.save):
        return 0
    if case.nt is not None:
        return int(case.nt != 0)
    return int(case.op == "bwd" and case.C >= 128 and M * 4 * case.C * 2 >= 256 << 20)


def plan_text(case, cus):
    """What mmg_cnblock_plan returns for the case on a device of `cus` CUs."""
    pl = plan(case, cus)
    b = block(case)
    b = f"({b[0]},{b[1]})" if case.op == "bwdw" else str(b)
    return f"{kernel_note(case)} grid={pl['grid']} block={b} lds={lds(case)} nt={nt(case, pl['M'])} tiles={pl['ntiles']}"


def plan_args(case, cus):
    """The arguments of mmg_cnblock_plan for the case."""
    return ({"fwd": 0, "bwd": 1, "bwdw": 2}[case.op], rows(case, cus), case.C, int(bool(case.save)) if case.op == "fwd" else 0,
            int(case.ln) if case.op == "bwd" else 0, cus)


def instantiations(case):
    """The kernel template instantiations a case launches (cnblock_bwdw: two)."""
    if case.op == "fwd":
        rw = resident(case)
        return [("cnblock_mlp_fwd_kernel", case.C, False, rw) if rw else ("cnblock_mlp_fwd_kernel", case.C, bool(case.save))]
    if case.op == "bwd":
        return [("cnblock_mlp_bwd_kernel", case.C, case.C != 384, case.ln)]
    var = 2 if case.var is None else case.var
    first = (1, 12, 0) if case.w12 else (1, 8, var if var in (1, 2) else 0)
    hto = 1 if case.hto is None else case.hto
    return [("cnblock_bwdw_kernel", 96) + first, ("cnblock_bwdw_kernel", 96, 2, 8, 1 if hto else 0)]


def _spell(args):
    return ", ".join(("true" if a else "false") if isinstance(a, bool) else str(a) for a in args)


def kernel_note(case):
    """mmg_last_kernel() after the case's launch."""
    inst = instantiations(case)
    if case.op == "bwdw":
        return f"cnblock_bwdw_kernel<{_spell(inst[0][1:])}> + <{_spell(inst[1][1:])}>"
    return f"{inst[0][0]}<{_spell(inst[0][1:])}>"


ALL_INSTANTIATIONS = (
    {("cnblock_mlp_fwd_kernel", C, s) for C in WIDTHS for s in (False, True)}
    | {("cnblock_mlp_fwd_kernel", 96, False, rw) for rw in (8, 12)}
    | {("cnblock_mlp_bwd_kernel", C, C != 384, ln) for C in BWD_WIDTHS for ln in (False, True)}
    | {("cnblock_bwdw_kernel", 96, 1, 8, v) for v in (0, 1, 2)} | {("cnblock_bwdw_kernel", 96, 1, 12, 0)}
    | {("cnblock_bwdw_kernel", 96, 2, 8, v) for v in (0, 1)})


# ---- the table -------------------------------------------------------------------------------------------------------------------
def _table():
    T = []
    for C in WIDTHS:
        edges = (1, 17, 16 * mt(C) + 1, BM - 1, BM + 1, 2 * BM + 16 * mt(C) + 3)
        for i, M in enumerate(edges):                     # every tail against every kind of output
            T.append(Case("fwd", C, M, "integer", save=(0, 1, 2, 3, 4, 1)[i], res=0 if C == 96 else None))
        T.append(Case("fwd", C, BM + 1, "integer", save=0, res=0 if C == 96 else None))
        T.append(Case("fwd", C, 17, "integer", save=4, nt=1))
        T.append(Case("fwd", C, 17, "integer", save=4, nt=0))
        T.append(Case("fwd", C, 2 * BM + 16 * mt(C) + 3, "gaussian", save=4, nt=1 if C == 192 else None))
        T.append(Case("fwd", C, BM - 1, "gaussian", save=0, res=0 if C == 96 else None))
        T.append(Case("fwd", C, 0, "integer", save=1 if C != 96 else 0, res=0 if C == 96 else None))      # the tile loop
    T.append(Case("fwd", 96, 0, "integer", save=3))
    T.append(Case("fwd", 128, 0, "gaussian", save=2))
    # the resident forward: 32-row wave tiles, rw waves per workgroup; 32 rw + 33 rows = rw + 2 tiles: the last workgroup has two waves
    # with a tile and rw - 2 without
    for rw in (8, 12):
        for M in (1, 17, 31, 33, 32 * rw - 1, 32 * rw + 1, 32 * rw + 33, 32 * (2 * rw + 1) + 19):
            T.append(Case("fwd", 96, M, "integer", res=rw))
        T.append(Case("fwd", 96, 32 * rw + 33, "gaussian", res=rw))
        T.append(Case("fwd", 96, 0, "integer", res=rw))
    T.append(Case("fwd", 96, 0, "gaussian"))                                  # (unset: 12 waves)
    for C in BWD_WIDTHS:
        edges = (1, 17, 16 * mt(C) + 1, BM - 1, BM + 1, 2 * BM + 16 * mt(C) + 3)
        for i, M in enumerate(edges):
            T.append(Case("bwd", C, M, "integer", ln=bool(i & 1)))
            T.append(Case("bwd", C, M, "integer", ln=not (i & 1), nt=i & 1))
        T.append(Case("bwd", C, 2 * BM + 16 * mt(C) + 3, "gaussian", ln=True))
        T.append(Case("bwd", C, BM - 1, "gaussian", ln=False, nt=1))
        T.append(Case("bwd", C, 0, "integer", ln=C == 128))
    T.append(Case("bwd", 96, 0, "gaussian", ln=True))
    for var in (0, 1, 2):
        for hto in (0, 1):
            T.append(Case("bwdw", 96, 128 if (var + hto) & 1 else 64, "integer", var=var, hto=hto))
    T.append(Case("bwdw", 96, 128, "integer", w12=1))
    T.append(Case("bwdw", 96, 64, "integer"))
    T.append(Case("bwdw", 96, 128, "gaussian"))
    T.append(Case("bwdw", 96, 64, "gaussian", w12=1, hto=0))
    T.append(Case("bwdw", 96, 128, "gaussian", var=0, hto=0))
    T.append(Case("bwdw", 96, 0, "integer"))
    T.append(Case("bwdw", 96, 0, "integer", var=0, hto=0))
    T.append(Case("bwdw", 96, 0, "gaussian"))
    return T


CASES = _table()


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _rb(x):
    """Round to bf16 (through fp32, as the kernels do), back in float64."""
    return x.to(torch.float32).to(BF).to(F64)


def _r32(x):
    return x.to(torch.float32).to(F64)


def half_ulp_bf16(v):
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 9)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def data_key(case):
    """What the operands depend on: (op, C, regime, base rows)."""
    return (case.op, case.C, case.regime, min(case.M, P) if case.M else P)


def make_data(case):
    """dict of float64 tensors for the base block of min(M, P) rows: bf16-exact xd / res / dy / W1 / W2, fp32-exact vectors."""
    op, C, regime, n = data_key(case)
    H4 = 4 * C
    g = torch.Generator().manual_seed(zlib.crc32(repr(data_key(case)).encode()))
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=F64)
    d = {}
    if regime == "integer":
        x = torch.ones(n, C, dtype=F64)
        for r in range(n):                                # an independent sign pattern per row, C/2 of each sign
            x[r, torch.randperm(C, generator=g)[:C // 2]] = -1.0
        keep = (torch.rand(H4, C, generator=g) < 0.25).to(F64)          # sparse, so that |h| stays below 256 at every width
        d.update(xd=x, eps=3.0, ln_w=ri(0, 1, C) * 2 + 2, ln_b=ri(-2, 2, C), w1=ri(0, 1, H4, C).mul(2).sub(1) * keep,
                 w2=ri(-1, 1, C, H4) * (torch.rand(C, H4, generator=g) < 0.25).to(F64), b2=ri(-3, 3, C), res=ri(-4, 4, n, C),
                 dy=ri(-1, 1, n, C), ls=2.0 ** ri(-1, 1, C))
        d["ln_w"] *= ri(0, 1, C) * 2 - 1
        # b1 per unit, distinct modulo 7, so large that |h| >= 8: s bounds |LN-out W1^T| for these rows (bwdw: xhat (W1 ln_w)^T + W1 ln_b)
        xln = 0.5 * x * d["ln_w"] + d["ln_b"]
        s = float((xln @ d["w1"].t()).abs().max())
        sign = torch.ones(H4, dtype=F64) if op == "bwd" else ri(0, 1, H4) * 2 - 1       # mlp_bwd: h >= 8 only
        d["b1"] = sign * (s + 8 + torch.arange(H4, dtype=F64) % 7)
    else:
        x = rn(n, C)
        if n >= 4:
            for r in range(n):
                if r % 8 == 1:
                    x[r] += 100.0
                elif r % 64 == 2:
                    x[r] = x[r, 0]
                elif r % 64 == 3:
                    x[r] *= 2.0 ** -20
        d.update(xd=_rb(x), eps=1e-6, ln_w=_r32(1 + 0.2 * rn(C)), ln_b=_r32(0.1 * rn(C)), w1=_rb(rn(H4, C) / C ** 0.5),
                 w2=_rb(rn(C, H4) / H4 ** 0.5), b1=_r32(0.1 * rn(H4)), b2=_r32(0.1 * rn(C)), res=_rb(rn(n, C)), dy=_rb(0.5 * rn(n, C)),
                 ls=_r32(0.3 + 0.7 * torch.rand(C, generator=g, dtype=F64)))
    # the images the kernels multiply by: the products in fp32 (one rounding), then bf16
    d["w2g"] = _rb(_r32(d["w2"] * d["ls"][:, None]))
    d["w1g"] = _rb(_r32(d["w1"] * d["ln_w"][None, :]))
    return d


def counts(M, n):
    """How often each of the n base rows occurs among M periodic rows."""
    return torch.bincount(torch.arange(M) % n, minlength=n).to(F64)


# ---- the arithmetic, row by row --------------------------------------------------------------------------------------------------
def _poly(x, coef):
    xc = x.clamp(-4.0, 4.0)
    u = xc * xc
    r = torch.full_like(x, coef[0])
    for c in coef[1:]:
        r = r * u + c
    t = 0.5 + xc * r
    return xc, torch.where(xc >= 4.0, torch.ones_like(t), torch.where(xc <= -4.0, torch.zeros_like(t), t))     # exact beyond the clamp


_T = (2.2038399460e-08, -1.5565415077e-06, 4.7013063952e-05, -8.0343697344e-04, 8.7106341480e-03, -6.4399300920e-02, 3.9770520692e-01)
_S = (-2.1511327673e-08, 1.5282923286e-06, -4.6282682125e-05, 7.8770984093e-04, -8.3827432669e-03, 5.8451897744e-02, -2.6627910133e-01,
      7.9896733648e-01)


def gelu_bf16(x):
    return x * _poly(x, _T)[1]


def gelu_bf16_grad_poly(x):
    return _poly(x, _S)[1]


def gelu_bf16_both_grad(x):
    xc, t = _poly(x, _T)
    return t + xc * torch.exp(-0.5 * xc * xc) * 0.3989422804014327


def unit_at_pos(n):
    """Hidden unit (output column) held at row position p of a packed image: 8q + 4tt + r at position 16 tt + 4q + r per 32."""
    p = torch.arange(n)
    return (p & ~31) + 8 * ((p >> 2) & 3) + 4 * ((p >> 4) & 1) + (p & 3)


def rowwise(case, d, contract, mut=None, stale=False):
    """Per base row, float64.  contract = False: the plain operation (erf GELU, no rounding inside).  contract = True: the kernels'
    rounding points and polynomial GELU forms, the weights through the packed images; mut / stale: see MUTATIONS."""
    C, H4, op = case.C, 4 * case.C, case.op
    rb = _rb if contract else (lambda t: t)
    integer = case.regime == "integer"
    x, eps = d["xd"], d["eps"]
    NC = 64 if C <= 128 else 32
    w1, w2, w2g, w1g, b1 = d["w1"], d["w2"], d["w2g"], d["w1g"], d["b1"]
    if contract and op != "bwdw":
        # through the packed images: position p of an A-type part holds unit_at_pos[p] (mlp_pack_kernel) and the lane that owns position
        # p takes it for unit_at_pos[p] (the kernels' n0 + 4 tt + r); B-type rows (output columns) by the same rule
        up = unit_at_pos(H4)
        held = up ^ 4 if mut == "pack_swap4" else up              # what the pack put at each position
        w1 = _scatter_cols(w1[held].t(), up).t()                  # [position] -> [unit] as the lanes read it
        w2g = _scatter_cols(w2g[:, held], up)
        if mut == "b1_packed":
            b1 = _scatter_cols(b1[None, :], up)[0]                # s_b1[position] taken for the unit's bias
    if contract and stale:
        # chunk 0 multiplied by the image of the LAST chunk (the ring buffer not refilled at a tile boundary)
        w1, w2, w2g, w1g = w1.clone(), w2.clone(), w2g.clone(), w1g.clone()
        w1[:NC], w2[:, :NC], w2g[:, :NC], w1g[:NC] = w1[H4 - NC:], w2[:, H4 - NC:], w2g[:, H4 - NC:], w1g[H4 - NC:]
    mean = x.sum(1) if mut == "mean_no_1_over_c" else x.mean(1)
    dd_ = x - mean[:, None]
    var = (dd_ * dd_).mean(1)
    rstd = (var + (0.0 if mut == "eps_dropped" else eps)) ** -0.5
    if contract:
        mean, rstd = _r32(mean), _r32(rstd)
    xhat = dd_ * rstd[:, None]
    xln = rb(xhat * d["ln_w"] + d["ln_b"])
    o = dict(mean=mean, rstd=rstd, xln=xln, xhat=xhat)
    sat = lambda h: torch.where(h > 0, h, torch.zeros_like(h))         # GELU beyond the clamp (integer regime: |h| >= 8)
    step = lambda h: (h > 0).to(F64)
    if op == "fwd":
        h = xln @ w1.t() + b1
        g = rb(gelu_bf16(h) if contract else (sat(h) if integer else gelu64(h)))
        dgp = gelu_bf16_grad_poly(h) if contract else (step(h) if integer else gelu_grad64(h))
        acc = g @ w2.t()
        if contract:
            # B-type rows: position p holds output column unit_at_pos[p], and the lane stores position p's sum to that column
            cp = unit_at_pos(C)
            held_c = torch.arange(C) if mut == "no_colperm" else cp
            acc = _scatter_cols(acc[:, held_c], cp)
        b2 = 0.0 if mut == "b2_dropped" else d["b2"]
        ls = 1.0 if mut == "ls_dropped" else d["ls"]
        res = 0.0 if mut == "res_dropped" else d["res"]
        o.update(h=h, hpre=rb(h), hpre1=rb(dgp), g_exact=g, gact=g, acc=acc, y=rb(res + ls * (acc + b2)))
        return o
    if op == "bwd":
        h = xln @ w1.t() + b1
        if C == 384:                                     # the saved pre-activation: the plain h, which the kernel reads back as bf16
            h = _rb(d["hsaved"]) if contract else d["hsaved"]
        gfun = (lambda t: gelu_bf16(t)) if contract else (sat if integer else gelu64)
        if contract:
            dgp = gelu_bf16_both_grad(-h if mut == "gelu_grad_sign" else h)
        else:
            dgp = step(h) if integer else gelu_grad64(h)
        dG = d["dy"] @ (d["w2"] if (mut == "ls_missing_dG" and contract) else w2g)
        dh = rb(dG * dgp)
        dx = dh @ w1
        o.update(h=h, g=rb(gfun(h)), dG=dG, dgp=dgp, dh=dh, dx=dx, dxln=rb(dx))
        if case.ln:
            o.update(_ln_bwd(dx * d["ln_w"], xhat, rstd, rb))
        return o
    # bwdw
    xhb = rb(xhat)
    b1f = d["b1"] + d["w1"] @ d["ln_b"]
    if contract:
        b1f = _r32(b1f)
    b1f_k = b1f + d["w1"] @ d["ln_b"] if mut == "b1f_twice" else b1f
    h = xhb @ w1g.t() + b1f_k
    g = rb(gelu_bf16(h) if contract else (sat(h) if integer else gelu64(h)))
    if contract:
        dgp = gelu_bf16_grad_poly(-h if mut == "gelu_grad_sign" else h)
    else:
        dgp = step(h) if integer else gelu_grad64(h)
    dG = d["dy"] @ (d["w2"] if (mut == "ls_missing_dG" and contract) else w2g)
    dh = dG * dgp
    dhb = rb(dh)
    dln = dhb @ d["w1"]
    o.update(xhb=xhb, b1f=b1f, h=h, g=g, dG=dG, dgp=dgp, dh=dh, dhb=dhb, dx=dln)
    o.update(_ln_bwd(dln * d["ln_w"], xhb, rstd, rb))
    return o


def _scatter_cols(t, idx):
    out = torch.empty_like(t)
    out[:, idx] = t
    return out


def _ln_bwd(q, xh, rstd, rb):
    m1, m2 = q.mean(1, keepdim=True), (q * xh).mean(1, keepdim=True)
    t = q - m1 - xh * m2
    return dict(q=q, m1=m1, m2=m2, t=t, dd=rb(rstd[:, None] * t))


def reduce_rows(case, d, o, w, fill=True, mut=None):
    """The accumulated outputs from per-row values o (row r weighing w[r]) plus the pre-fill."""
    f = (lambda k: FILL[k]) if fill else (lambda k: 0.0)
    wc = w[:, None]
    if case.op == "bwd":
        if not case.ln:
            return {}
        return dict(ln_dw=(wc * o["dx"] * o["xhat"]).sum(0) + f("ln_dw"), ln_db=(wc * o["dx"]).sum(0) + f("ln_db"))
    if case.op != "bwdw":
        return {}
    db1 = (wc * o["dh"]).sum(0)
    raw = (wc * o["dhb"]).t() @ o["xhb"]
    dW1 = d["ln_w"][None, :] * raw + (0.0 if mut == "dW1_no_db1_term" else db1[:, None] * d["ln_b"][None, :])
    return dict(dW2raw=(wc * d["dy"][:len(w)]).t() @ o["g"] + f("dW2raw"), db2raw=(wc * d["dy"][:len(w)]).sum(0) + f("db2raw"),
                db1=db1 + f("db1"), dW1=dW1 + f("dW1"), ln_dw=(wc * o["dx"] * o["xhb"]).sum(0) + f("ln_dw"),
                ln_db=(wc * o["dx"]).sum(0) + f("ln_db"))


ROW_OUTPUTS = {"fwd": ("y", "hpre", "xln", "gact", "mean", "rstd"), "bwd": ("g", "dh", "xln", "dxln", "mean", "rstd"), "bwdw": ("dd",)}
ACC_OUTPUTS = {"fwd": (), "bwd": ("ln_dw", "ln_db"), "bwdw": ("dW1", "db1", "dW2raw", "db2raw", "ln_dw", "ln_db")}


def outputs_of(case):
    """Names of the outputs a case's launch writes (row outputs, accumulated outputs)."""
    if case.op == "fwd":
        r = ("y",) + (("hpre", "mean", "rstd") if case.save else ()) + (("xln",) if case.save >= 2 else ()) + (("gact",) if case.save >= 3 else ())
        return r, ()
    if case.op == "bwd":
        return ROW_OUTPUTS["bwd"], (ACC_OUTPUTS["bwd"] if case.ln else ())
    return ("dd", "b1f"), ACC_OUTPUTS["bwdw"]


def exact_outputs(case):
    """Outputs compared with torch.equal (integer regime; see the module docstring for the split)."""
    if case.regime != "integer":
        return ()
    if case.op == "fwd":
        return ("y", "hpre", "xln", "gact", "mean")
    if case.op == "bwd":
        return ("g", "dh", "xln", "mean", "ln_db") + (() if case.ln else ("dxln",))
    return ("b1f", "dW1", "db1", "dW2raw", "db2raw", "ln_dw", "ln_db")


# ---- reference and bars ----------------------------------------------------------------------------------------------------------
def reference(case, d, M):
    """-> (ref, bar): {output: float64 tensor} for the base rows (row outputs) / the whole launch of M rows (accumulated outputs).
    integer regime: the reference follows the (exactly known) bf16 roundings, and the bf16 terms of the bars are zero."""
    integer = case.regime == "integer"
    n = d["xd"].shape[0]
    w = counts(M, n)
    o = _integer_rowwise(case, d) if integer else rowwise(case, d, contract=False)
    u8 = 0.0 if integer else U8
    ge = 0.0 if integer else 1.0
    C, H4, u = case.C, 4 * case.C, U32
    x = d["xd"]
    A = torch.abs
    # LayerNorm
    e_mean = K_ACC * u * A(x).mean(1)
    dev_ = x - x.mean(1, keepdim=True)
    var = (dev_ * dev_).mean(1)
    rstd = o["rstd"]
    e_rstd = 0.5 * rstd ** 3 * (2 * A(dev_).mean(1) * e_mean + e_mean ** 2 + K_ACC * u * (var + d["eps"])) + K_ACC * u * rstd
    xhat = o["xhat"]
    e_xhat = rstd[:, None] * (e_mean[:, None] + 2 * u * A(dev_)) + A(dev_) * e_rstd[:, None]
    e_xln = A(d["ln_w"]) * e_xhat + 2 * u * (A(xhat * d["ln_w"]) + A(d["ln_b"]))
    hu = half_ulp_bf16
    ref = dict(mean=o["mean"], rstd=o["rstd"], xln=o["xln"])
    bar = dict(mean=e_mean, rstd=e_rstd, xln=hu(o["xln"]) + e_xln)
    eop_xln = ge * (u8 * A(o["xln"]) + e_xln)
    wc = w[:, None]

    def gelu_err(h, g, e_h):
        return LIP1 * e_h + ge * (GELU_REL * (A(g) + LIP1 * e_h) + GELU_NEG * (h < e_h).to(F64)) + u * A(g)

    def ln_bwd_bar(dx, e_dx, xh, e_x):
        q = o["q"]
        e_q = A(d["ln_w"]) * e_dx + u * A(q)
        e_m1 = e_q.mean(1, keepdim=True) + kd(C) * u * A(q).mean(1, keepdim=True)
        e_m2 = (e_q * A(xh) + A(q) * e_x).mean(1, keepdim=True) + kd(C) * u * A(q * xh).mean(1, keepdim=True)
        e_t = e_q + e_m1 + A(xh) * e_m2 + A(o["m2"]) * e_x + 3 * u * (A(q) + A(o["m1"]) + A(xh * o["m2"]))
        return hu(o["dd"]) + rstd[:, None] * e_t + e_rstd[:, None] * A(o["t"]) + u * A(o["dd"])

    def acc_bar(name, operand, mag):
        return operand + K_ACC * u * (mag + abs(FILL[name]))

    if case.op == "fwd":
        aw1, aw2 = A(d["w1"]), A(d["w2"])
        e_h = eop_xln @ aw1.t() + kd(C) * u * (A(o["xln"]) @ aw1.t() + A(d["b1"]))
        e_g = gelu_err(o["h"], o["g_exact"], e_h)
        eop_g = ge * (u8 * A(o["gact"]) + e_g)
        e_acc = eop_g @ aw2.t() + kd(H4) * u * (A(o["gact"]) @ aw2.t())
        e_y = A(d["ls"]) * (e_acc + u * (A(o["acc"]) + A(d["b2"]))) + 2 * u * (A(d["res"]) + A(d["ls"] * (o["acc"] + d["b2"])))
        ref.update(y=o["y"], hpre=o["hpre1"] if case.save == 4 else o["hpre"], gact=o["gact"])
        bar.update(y=hu(o["y"]) + e_y, gact=hu(o["gact"]) + e_g,
                   hpre=hu(o["hpre1"]) + LIP2 * e_h + GELUP_ABS if case.save == 4 else hu(o["hpre"]) + e_h)
        return ref, bar
    if case.op == "bwd":
        aw1 = A(d["w1"])
        if C == 384:
            e_h = ge * u8 * A(o["h"])
        else:
            e_h = eop_xln @ aw1.t() + kd(C) * u * (A(o["xln"]) @ aw1.t() + A(d["b1"]))
        e_g = gelu_err(o["h"], o["g"], e_h)
        e_dG = kd(C) * u * (A(d["dy"]) @ A(d["w2g"]))
        e_dgp = LIP2 * e_h + ge * GELUP_ABS
        e_dh = A(o["dG"]) * e_dgp + e_dG * (A(o["dgp"]) + e_dgp) + u * A(o["dh"])
        eop_dh = ge * (u8 * A(o["dh"]) + e_dh)
        e_dx = eop_dh @ aw1 + kd(H4) * u * (A(o["dh"]) @ aw1)
        ref.update(g=o["g"], dh=o["dh"])
        bar.update(g=hu(o["g"]) + e_g, dh=hu(o["dh"]) + e_dh)
        if not case.ln:
            ref["dxln"], bar["dxln"] = o["dxln"], hu(o["dxln"]) + e_dx
            return ref, bar
        ref["dxln"], bar["dxln"] = o["dd"], ln_bwd_bar(o["dx"], e_dx, xhat, e_xhat)
        ref.update(reduce_rows(case, d, o, w))
        bar["ln_dw"] = acc_bar("ln_dw", (wc * (e_dx * A(xhat) + A(o["dx"]) * e_xhat)).sum(0), (wc * A(o["dx"] * xhat)).sum(0))
        bar["ln_db"] = acc_bar("ln_db", (wc * e_dx).sum(0), (wc * A(o["dx"])).sum(0))
        return ref, bar
    # bwdw
    aw1, aw1g = A(d["w1"]), A(d["w1g"])
    xhb = o["xhb"]
    eop_xh = ge * (u8 * A(xhat) + e_xhat)
    e_b1f = kd(C) * u * (A(d["b1"]) + aw1 @ A(d["ln_b"]))
    e_h = eop_xh @ aw1g.t() + kd(C) * u * (A(xhb) @ aw1g.t() + A(o["b1f"])) + e_b1f
    e_g = gelu_err(o["h"], o["g"], e_h)
    eop_g = ge * (u8 * A(o["g"]) + e_g)
    e_dG = kd(C) * u * (A(d["dy"]) @ A(d["w2g"]))
    e_dgp = LIP2 * e_h + ge * GELUP_ABS
    e_dh = A(o["dG"]) * e_dgp + e_dG * (A(o["dgp"]) + e_dgp) + u * A(o["dh"])
    eop_dh = ge * (u8 * A(o["dh"]) + e_dh)
    e_dln = eop_dh @ aw1 + kd(H4) * u * (A(o["dh"]) @ aw1)
    ady = A(d["dy"])
    ref = dict(dd=o["dd"], b1f=o["b1f"])
    ref.update(reduce_rows(case, d, o, w))
    bar = dict(dd=ln_bwd_bar(o["dx"], e_dln, xhb, eop_xh), b1f=e_b1f)
    bar["dW2raw"] = acc_bar("dW2raw", (wc * ady).t() @ eop_g, (wc * ady).t() @ A(o["g"]))
    bar["db2raw"] = acc_bar("db2raw", 0.0, (wc * ady).sum(0))
    db1_op, db1_mag = (wc * e_dh).sum(0), (wc * A(o["dh"])).sum(0)
    bar["db1"] = acc_bar("db1", db1_op, db1_mag)
    raw_op = (wc * eop_dh).t() @ (A(xhb) + eop_xh) + (wc * A(o["dh"])).t() @ eop_xh
    raw_mag = (wc * A(o["dh"])).t() @ A(xhb)
    alw, alb = A(d["ln_w"])[None, :], A(d["ln_b"])[None, :]
    bar["dW1"] = acc_bar("dW1", alw * raw_op + alb * (db1_op + K_ACC * u * db1_mag)[:, None], alw * raw_mag + alb * db1_mag[:, None])
    bar["ln_db"] = acc_bar("ln_db", (wc * e_dln).sum(0), (wc * A(o["dx"])).sum(0))
    bar["ln_dw"] = acc_bar("ln_dw", (wc * (e_dln * A(xhb) + A(o["dx"]) * eop_xh)).sum(0), (wc * A(o["dx"] * xhb)).sum(0))
    return ref, bar


def _integer_rowwise(case, d):
    """The integer regime's reference: exact arithmetic with the three kinds of bf16 rounding applied to exactly known values and
    GELU / GELU' beyond the clamp (x or 0, 1 or 0)."""
    o = rowwise(case, d, contract=False)
    # (contract = False computes exactly; what is left is to round the stored values)
    C = case.C
    sat = lambda h: torch.where(h > 0, h, torch.zeros_like(h))
    if case.op == "fwd":
        xln = _rb(o["xln"])
        h = xln @ d["w1"].t() + d["b1"]
        g = _rb(sat(h))
        acc = g @ d["w2"].t()
        o.update(xln=xln, h=h, hpre=_rb(h), hpre1=(h > 0).to(F64), g_exact=g, gact=g, acc=acc, y=_rb(d["res"] + d["ls"] * (acc + d["b2"])))
    elif case.op == "bwd":
        xln = _rb(o["xln"])
        h = _rb(d["hsaved"]) if C == 384 else xln @ d["w1"].t() + d["b1"]
        dh = _rb(o["dG"] * (h > 0).to(F64))
        dx = dh @ d["w1"]
        o.update(xln=xln, h=h, g=_rb(sat(h)), dh=dh, dx=dx, dxln=_rb(dx))
        if case.ln:
            o.update(_ln_bwd(dx * d["ln_w"], o["xhat"], o["rstd"], lambda t: t))
    else:
        xhb = _rb(o["xhat"])
        h = xhb @ d["w1g"].t() + o["b1f"]
        dh = o["dG"] * (h > 0).to(F64)
        dhb = _rb(dh)
        dln = dhb @ d["w1"]
        o.update(xhb=xhb, h=h, g=_rb(sat(h)), dh=dh, dhb=dhb, dx=dln)
        o.update(_ln_bwd(dln * d["ln_w"], xhb, o["rstd"], lambda t: t))
    return o


@functools.lru_cache(maxsize=4)
def _prepared(key, M, case):
    d = make_data(case)
    if case.op == "bwd" and case.C == 384:          # the pre-activation the forward would have saved: the plain h (the kernel reads its bf16)
        o = rowwise(case._replace(op="fwd", save=1), d, contract=False)
        d["hsaved"] = _rb(o["xln"]) @ d["w1"].t() + d["b1"] if case.regime == "integer" else o["h"]
    ref, bar = reference(case, d, M)
    return d, ref, bar


def prepared(case, cus=256):
    """(data, reference, bars) of a case: computed once per (data, M, ln / save kind) and shared (callers must not modify them)."""
    M = rows(case, cus)
    # (the reference holds every optional output; only hpre's kind changes it)
    canon = case._replace(res=None, nt=None, var=None, hto=None, w12=None, M=M, save=4 if case.save == 4 else 3 if case.save else 0)
    return _prepared((data_key(case), M, canon.ln, canon.save), M, canon)


# ---- preconditions of the integer regime, on the reference alone -----------------------------------------------------------------
def exactness_violations(case, d, M):
    """Why torch.equal would NOT be justified for this integer case (empty list: it is)."""
    bad = []
    o = _integer_rowwise(case, d)
    w = counts(M, d["xd"].shape[0])[:, None]
    A = torch.abs
    half = lambda t: bool((2 * t == (2 * t).round()).all())
    x = d["xd"]
    if not (bool((A(x) == 1).all()) and bool((x.sum(1) == 0).all()) and d["eps"] == 3.0):
        bad.append("rows are not +-1 with C/2 of each sign at eps = 3")
    if not torch.equal(o["rstd"], torch.full_like(o["rstd"], 0.5)):
        bad.append("rstd is not 1/2")
    if not (half(o["xln"]) and float(A(o["xln"]).max()) <= 64):
        bad.append("the LayerNorm output is not a small integer (a few fp32 ulps of rstd must vanish in its bf16 rounding)")
    if not bool((A(o["h"]) >= 8).all()):
        bad.append("|h| < 8 somewhere")
    if case.op == "bwd" and not bool((o["h"] >= 8).all()):
        bad.append("mlp_bwd needs h >= 8 (GELU' = 1.0005 above the clamp, -5.4e-4 dG below)")
    if len(set((d["b1"].abs() % 7).tolist())) != 7:
        bad.append("b1 is not distinct modulo 7")
    if not half(o["h"]) or float(A(o["h"]).max()) >= 2 ** 24:
        bad.append("h is not an integer")
    sums = []
    if case.op == "fwd":
        sums += [A(o["xln"]) @ A(d["w1"]).t() + A(d["b1"]), A(o["gact"]) @ A(d["w2"]).t(), A(d["res"]) + A(d["ls"]) * (A(o["acc"]) + A(d["b2"]))]
        if not half(d["res"] + d["ls"] * (o["acc"] + d["b2"])):
            bad.append("y is not a multiple of 1/2 before its rounding")
    else:
        dG = o["dG"]
        for f in (1.00050, 1.00057):                     # GELU' of gelu_bf16_both above the clamp: 1 + 4 exp(-8) / sqrt(2 pi) = 1.000535
            if case.op == "bwd" and not torch.equal(_rb(dG * f), _rb(dG)):
                bad.append(f"bf16(dG x {f}) != bf16(dG)")
        sums += [A(d["dy"]) @ A(d["w2g"]), A(o["dh"]) @ A(d["w1"])]
        if not half(dG):
            bad.append("dG is not a multiple of 1/2")
        if case.op == "bwd" and case.ln:
            sums += [(w * A(o["dx"])).sum(0) + 1]
        if case.op == "bwdw":
            if not bool((A(o["xhb"]) == 0.5).all()):
                bad.append("bf16(xhat) is not +-1/2")
            if not torch.equal(_rb(d["w1"] * d["ln_w"]), d["w1"] * d["ln_w"]) or not half(o["b1f"]):
                bad.append("W1 ln_w is not bf16-exact / b1f is not an integer")
            sums += [(w * A(d["dy"])).t() @ A(o["g"]) + 1, (w * A(o["dh"])).sum(0) + 1, (w * A(o["dx"])).sum(0) + 1,
                     A(d["ln_w"])[None, :] * ((w * A(o["dhb"])).t() @ A(o["xhb"])) + A(d["ln_b"])[None, :] * (w * A(o["dh"])).sum(0)[:, None] + 1]
            if not (half(2 * o["dx"]) and half(o["dh"])):
                bad.append("dh / d LN-out are not multiples of 1/2 (1/4)")
    if any(float(s.max()) >= 2 ** 23 for s in sums):     # (2^23: multiples of 1/2 keep one bit below the point)
        bad.append("a partial sum could pass 2^23")
    return bad


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def check(case, name, got, ref, bar, exact=None):
    """got against ref (float64, same shape) -> (worst ratio to the bar, share of elements that differ from the reference cast to the
    output type).  Exact outputs: the ratio is 0.0 (equal) or inf."""
    is_bf = name not in ("mean", "rstd", "b1f") + ACC_OUTPUTS["bwdw"]
    cast = _rb(ref) if is_bf else _r32(ref)
    differ = (got != cast).double().mean().item()
    if not torch.isfinite(got).all():
        return float("inf"), differ
    if name in (exact_outputs(case) if exact is None else exact):
        return (0.0 if differ == 0 else float("inf")), differ
    diff = (got - ref).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bar)
    return ratio.max().item(), differ


# ---- emulation of the launch, and mutations of it --------------------------------------------------------------------------------
MUTATIONS = ("pack_swap4", "no_colperm", "b1_packed", "b2_dropped", "ls_dropped", "res_dropped", "eps_dropped", "mean_no_1_over_c",
             "stale_chunk", "tile_skipped", "clamp_leak", "tail_rows_counted", "last_block_unwritten", "b1f_twice", "dW1_no_db1_term",
             "ls_missing_dG", "gelu_grad_sign")


def mutation_applies(case, mut, cus=256):
    """Whether the case contains the feature a mutation breaks."""
    pl = plan(case, cus)
    M = pl["M"]
    fwd, bwd, bwdw = (case.op == o for o in ("fwd", "bwd", "bwdw"))
    recomputes = not (bwd and case.C == 384)
    return {
        "pack_swap4": not bwdw,
        "no_colperm": fwd,
        "b1_packed": not bwdw and recomputes,
        "b2_dropped": fwd, "ls_dropped": fwd, "res_dropped": fwd,
        "eps_dropped": case.regime == "gaussian" and M >= 4,               # the constant row: var = 0
        "mean_no_1_over_c": case.regime == "gaussian",                     # (integer rows sum to zero: the mean is 0 either way)
        "stale_chunk": not bwdw and not resident(case) and pl["max_tiles"] >= 2,
        "tile_skipped": pl["max_tiles"] >= 2,
        "clamp_leak": not bwdw and M >= 2,
        "tail_rows_counted": bwd and case.ln and M % BM != 0,
        "last_block_unwritten": not bwdw,
        "b1f_twice": bwdw, "dW1_no_db1_term": bwdw,
        "ls_missing_dG": not fwd,
        "gelu_grad_sign": not fwd,
    }[mut]


def emulate(case, d, cus=256, mut=None):
    """The launch over all M rows -> {output: float64}; unwritten elements stay NaN.  mut: one of MUTATIONS."""
    pl = plan(case, cus)
    M, tile, walkers = pl["M"], pl["tile"], pl["walkers"]
    n = d["xd"].shape[0]
    src = torch.arange(M) % n                              # the base row each row reads
    if mut == "clamp_leak":
        src[M - 1] = (M - 2) % n                           # the clamp one row short: the last row reads row M - 2
    o = rowwise(case, d, contract=True, mut=mut)
    which = torch.zeros(M, dtype=torch.bool)               # rows of a walker's second tile
    if mut == "stale_chunk":
        o2 = rowwise(case, d, contract=True, stale=True)
        t = torch.arange(M) // tile
        which = (t >= walkers) & (t < 2 * walkers)
    skipped = torch.zeros(M, dtype=torch.bool)
    if mut == "tile_skipped":
        t = torch.arange(M) // tile
        skipped = t == walkers                             # the second tile of walker 0
    if mut == "last_block_unwritten":
        skipped = torch.arange(M) >= (M - 1) // 16 * 16
    rows_out, accs = outputs_of(case)
    out = {}
    key = {"hpre": "hpre1" if case.save == 4 else "hpre", "dxln": "dd" if case.ln else "dxln"}

    def full(name):
        v = o[key.get(name, name)][src]
        if which.any():
            v = torch.where(which.reshape(-1, *[1] * (v.dim() - 1)), o2[key.get(name, name)][src], v)
        return v
    for name in rows_out:
        if name == "b1f":
            out[name] = o["b1f"] + (d["w1"] @ d["ln_b"] if mut == "b1f_twice" else 0.0)
            continue
        v = full(name).clone()
        v[skipped] = float("nan")
        out[name] = v
    if accs:
        per = {k: full(k) for k in (("dx", "xhat") if case.op == "bwd" else ("dh", "dhb", "xhb", "g", "dx"))}
        w = (~skipped).to(F64) if mut == "tile_skipped" else torch.ones(M, dtype=F64)
        dfull = dict(d, dy=d["dy"][src])
        if mut == "tail_rows_counted":                     # rows M .. up to the end of the last tile, read from row M - 1, counted too
            extra = cdiv(M, BM) * BM - M
            w = w.clone()
            w[M - 1] += extra
        acc = reduce_rows(case, dfull, per, w, mut=mut)
        out.update({k: _r32(v) for k, v in acc.items()})
    return out


def expand(case, ref, bar, M):
    """Reference and bars of the row outputs for all M rows (small M only: the CPU tests and the non-loop GPU cases)."""
    n = next(v.shape[0] for k, v in ref.items() if k in ("dd", "xln"))
    src = torch.arange(M) % n
    rows_out, _ = outputs_of(case)
    pick = lambda t, k: t[k][src] if k in rows_out and k != "b1f" else t[k]
    return {k: pick(ref, k) for k in ref}, {k: pick(bar, k) for k in bar}
