"""Float64 reference, derived error bars and a kernel emulation (with mutations) for the attention kernels of csrc/attention.hip.

Imported by tests/test_attention_ref_cpu.py (no GPU: the bars hold for the emulation and every mutation of it is caught) and by
tests/test_attention_gpu.py (the kernels against the same bars).  Everything here runs on the CPU in float64 from bf16-exact inputs.

All tensors are per head: q, k, v, dO [B, heads, S, 64] float64; `valid` [B, S] bool marks the attended keys (any pattern; for the
packed layout key < length, and the rows past a sequence's length hold zeros and are never compared).

Error model.  A kernel rounds exactly one operand to bf16 between its two matrix products (the probabilities before P V and
P^T dO, dS before dS K and dS^T Q) and its output once more.  Everything else is fp32 accumulation and the hardware exp / exp2 / log,
orders of magnitude below a bf16 rounding.  So every bar is  |got - bf16(ref)| <= ulp_bf16(ref) + A  with A = U * sum |rounded operand|
|other operand|, U = 2^-8: the half ulp 2^-9 of that one rounding, and a spare 2^-9 for the fp32 part.  The bars come from the float64
reference alone."""
import functools
import math
import zlib
from typing import NamedTuple

import numpy as np
import torch

from oracle import dropout_oracle as D

BF = torch.bfloat16
F64 = torch.float64
U = 2.0 ** -8            # twice the half ulp of the one bf16 rounding between a kernel's two matrix products (see above)
HALF = 2.0 ** -9         # relative half ulp of a bf16 rounding
U32 = 2.0 ** -24         # unit round-off of fp32
# lse bar: K_LSE 2^-24 (scale max_k sum_d |q_d k_d| + |lse| + 1).  K_LSE depends on the hardware exp and log, so it is measured:
# the smallest power of two >= 4 x the worst ratio recorded on an MI355X over every case of CASES with K_LSE = 1
# (profiles/attention_measured_tolerances.jsonl, field lse_ratio_k1; DESIGN.md "Attention kernels against float64").
K_LSE = 8.0
# fp32 terms of a probability itself (read-out cases, where the bf16 allowance is zero): the score is a 64-term fp32 dot product and
# exp multiplies an absolute error of its argument into a relative one of its value; 8 x 2^-24 (scale sum|q k| + |lse| + 1) per
# probability is a loose bound of that and still 2^-13 of a bf16 ulp at the magnitudes of these tests.
K_EXP = 8.0
SEED, SITE = 99, 5       # dropout mask of every DROP case
NONPOW2_SCALE = float(np.float32(1.0 / math.sqrt(128.0)))


class Case(NamedTuple):
    family: str                    # whole | packed | tiled | drop | drop_packed
    S: int                         # sequence length (packed: S_max)
    regime: str                    # flat | peaked | offset | ascending | descending | readout
    mask: str = "none"             # none | right | left | holes   (packed: lengths instead)
    B: int = 2
    heads: int = 2
    scale: float = 0.125
    wide: bool = False             # leading dimensions wider than the minimum, each a different multiple of 8
    rb: int = 0                    # MMG_ATT_RB (tiled forward / dQ), 0 = unset
    rbk: int = 0                   # MMG_ATT_RB_DKV (tiled dK/dV)
    p: float = 0.0                 # dropout probability
    window: int = 0                # read-out: first key / query of the 64-wide identity window

    @property
    def id(self):
        s = f"{self.family}-S{self.S}-{self.regime}-{self.mask}-bh{self.B}x{self.heads}"
        if self.rb:
            s += f"-rb{self.rb}{self.rbk}"
        if self.p:
            s += "-drop"
        if self.wide:
            s += "-wide"
        if self.scale != 0.125:
            s += "-scale"
        if self.regime == "readout":
            s += f"-w{self.window}"
        return s

    @property
    def lens(self):
        """Packed layout: the sequence lengths (S_max, 33, 1)."""
        return [self.S, 33, 1] if self.family in ("packed", "drop_packed") else None

    @property
    def has_bwd(self):
        return self.family in ("tiled", "drop") or self.S <= 256


def _table():
    C = []

    def add(family, S, regime, mask="none", **kw):
        if family in ("packed", "drop_packed"):
            kw.setdefault("B", 3)
        C.append(Case(family, S, regime, mask, **kw))

    # whole-sequence kernels: NT = 6 (S_pad/16 <= 6: S = 1, 19, 96), 8 (97), 16 (129), 32 (257, 512); backward up to S = 256
    add("whole", 1, "flat")
    add("whole", 19, "flat", "right")
    add("whole", 19, "peaked", "holes")
    add("whole", 96, "flat")
    add("whole", 96, "peaked", "left")
    add("whole", 96, "readout", window=16)
    add("whole", 97, "flat", "right")
    add("whole", 97, "peaked", "holes")
    add("whole", 97, "readout", "left", window=33)
    add("whole", 97, "flat", "holes", wide=True, scale=NONPOW2_SCALE)
    add("whole", 97, "offset", "right")
    add("whole", 129, "flat", "left")
    add("whole", 129, "peaked")
    add("whole", 129, "readout", "holes", window=64)
    add("whole", 256, "flat", "right")
    add("whole", 256, "peaked", "left")
    add("whole", 256, "readout", window=100)
    add("whole", 257, "flat", "holes")
    add("whole", 257, "peaked", "right")
    add("whole", 257, "readout", window=193)
    add("whole", 512, "flat")
    add("whole", 512, "peaked", "left")
    # packed layout, lengths (S_max, 33, 1)
    add("packed", 77, "flat")
    add("packed", 77, "peaked", wide=True, scale=NONPOW2_SCALE)
    add("packed", 77, "readout", window=5)
    add("packed", 256, "flat", wide=True)
    add("packed", 256, "peaked")
    # tiled kernels: every S x every rows-per-wave pair in the flat regime, the masks taken in turn
    pairs = [(1, 1), (2, 2), (4, 3)]
    masks = ["none", "right", "left", "holes"]
    i = 0
    for S in (63, 64, 65, 130, 300):
        for rb, rbk in pairs:
            add("tiled", S, "flat", masks[i % 4], rb=rb, rbk=rbk)
            i += 1
    # peaked and read-out for every instantiation (RB x MASK); one window inside a 64-key tile, one straddling a tile boundary
    for j, (rb, rbk) in enumerate(pairs):
        add("tiled", 130, "peaked", rb=rb, rbk=rbk)
        add("tiled", (65, 130, 300)[j], "peaked", "left", rb=rb, rbk=rbk)
        add("tiled", (300, 130, 300)[j], "readout", rb=rb, rbk=rbk, window=(64, 40, 100)[j])
        add("tiled", (130, 300, 130)[j], "readout", ("holes", "left", "right")[j], rb=rb, rbk=rbk, window=(40, 128, 64)[j])
    # the online softmax at work: running maximum far from zero / moving in every tile / never moving after the first
    add("tiled", 300, "offset", rb=1, rbk=1)
    add("tiled", 300, "offset", "left", rb=4, rbk=3)
    add("tiled", 300, "ascending", rb=2, rbk=2)
    add("tiled", 300, "ascending", "right", rb=1, rbk=1)
    add("tiled", 300, "descending", rb=4, rbk=3)
    add("tiled", 300, "descending", "holes", rb=2, rbk=2)
    # workgroup maps: B x heads = 8 takes the XCD-grouped map, 4 (everything above) the plain one
    add("tiled", 130, "flat", "left", heads=4, rb=2, rbk=2)
    add("tiled", 300, "peaked", heads=4, rb=1, rbk=3)
    # wider leading dimensions and a scale that is no power of two
    add("tiled", 65, "flat", "right", rb=1, rbk=2, wide=True, scale=NONPOW2_SCALE)
    add("tiled", 300, "flat", rb=4, rbk=1, wide=True, scale=NONPOW2_SCALE)
    # dropout: DROP forward for every NT; whole-sequence DROP backward up to 256, the tiled DROP dQ / dK,dV (MASK on and off) beyond
    for S, ms, w in ((96, ("none", "right", "holes"), 32), (97, ("right", "left", "none"), 20), (129, ("holes", "none", "right"), 65),
                     (257, ("right", "none", "holes"), 150), (512, ("none", "left", "none"), 300)):
        add("drop", S, "flat", ms[0], p=0.1)
        add("drop", S, "peaked", ms[1], p=0.1)
        add("drop", S, "readout", ms[2], p=0.1, window=w)
    add("drop", 257, "flat", "left", p=0.1, wide=True, scale=NONPOW2_SCALE)
    add("drop_packed", 97, "flat", p=0.1)
    add("drop_packed", 97, "peaked", p=0.1, wide=True)
    return C


CASES = _table()


def instantiations(case):
    """The kernel template instantiations a case runs (att_launch_* in csrc/attention.hip)."""
    drop, masked = case.p > 0, case.mask != "none"
    if case.family == "tiled":
        return [("flash_fwd", case.rb, masked), ("flash_dq", case.rb, masked, False), ("flash_dkv", case.rbk, masked, False)]
    nt = -(-case.S // 32) * 2
    out = [("fwd", 6 if nt <= 6 else 8 if nt <= 8 else 16 if nt <= 16 else 32, drop)]
    if case.S <= 256:
        out.append(("bwd", drop))
    elif case.family == "drop":
        out += [("flash_dq", 2, masked, True), ("flash_dkv", 2, masked, True)]
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _rb(x):
    """Round to bf16, back in float64."""
    return x.to(torch.float32).to(BF).to(F64)


def bf16_ulp(v):
    """Spacing of bf16 numbers at |v| (float64 in and out); the smallest normal's spacing below that."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 8)


def make_valid(case):
    B, S = case.B, case.S
    g = torch.Generator().manual_seed(zlib.crc32(("mask" + case.id).encode()))
    k = torch.arange(S)[None, :]
    if case.lens is not None:
        return k < torch.tensor(case.lens)[:, None]
    if case.mask == "none":
        return torch.ones(B, S, dtype=torch.bool)
    if case.mask == "right":                                  # right-padded prefixes, the last one of length 1
        lens = [max(1, (S * 5) // 8 - b) for b in range(B - 1)] + [1]
        return k < torch.tensor(lens)[:, None]
    if case.mask == "left":                                   # at least 64 leading masked keys wherever S allows it
        lead = [min(S - 1, 64 + 66 * (b % 2)) if S > 64 else S // 2 + b for b in range(B)]
        return k >= torch.tensor(lead)[:, None]
    assert case.mask == "holes"
    v = torch.rand(B, S, generator=g) < 0.6
    v[torch.arange(B), torch.randint(0, S, (B,), generator=g)] = True       # at least one attended key per row
    return v


def make_inputs(case):
    """q, k, v, dO [B, heads, S, 64] float64 holding bf16-exact values; valid [B, S]; rows [B, S] (rows that exist: all but the tail
    of a packed sequence); keep [B, heads, S, S] or None."""
    B, H, S = case.B, case.heads, case.S
    g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    q, k, v, dO = [torch.randn(B, H, S, 64, generator=g, dtype=F64) for _ in range(4)]
    kk = torch.arange(S, dtype=F64)
    if case.regime == "peaked":                               # row maxima of the scaled scores in the tens: a few keys carry a row
        q = q * 4
    elif case.regime == "offset":                             # 4 x 16 x 12.5 = 800: every scaled score about +100 (at 1/8)
        q[..., :4] = 16.0
        k[..., :4] = 12.5
    elif case.regime in ("ascending", "descending"):          # scaled score + (-) key / 4 through column 0 (at 1/8)
        q[..., 0] = 16.0
        k[..., 0] = (kk if case.regime == "ascending" else -kk)[None, None, :] / 8
    elif case.regime == "readout":                            # ctx = a 64-key window of P; dV = a 64-query window of P^T
        w = case.window
        assert w + 64 <= S
        v = torch.zeros_like(v)
        dO = torch.zeros_like(dO)
        v[:, :, w:w + 64] = torch.eye(64, dtype=F64)
        dO[:, :, w:w + 64] = torch.eye(64, dtype=F64)
    valid = make_valid(case)
    rows = torch.ones(B, S, dtype=torch.bool)
    if case.lens is not None:
        rows = valid.clone()
        for t in (q, k, v, dO):
            t *= rows[:, None, :, None]
    keep = None
    if case.p:
        keep = torch.from_numpy(D.attention_mask(B, H, S, case.p, SEED, SITE).astype(np.bool_))
    return dict(q=_rb(q), k=_rb(k), v=_rb(v), dO=_rb(dO), valid=valid, rows=rows, keep=keep)


def _drop_scale(p):
    return 1.0 / (1.0 - float(np.float32(p))) if p else 1.0


# ---- float64 reference -----------------------------------------------------------------------------------------------------------
def _softmax(q, k, valid, scale):
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    return s, e / l, (m + torch.log(l)).squeeze(-1)


def reference(inp, scale, p=0.0):
    q, k, v, dO, valid, keep = inp["q"], inp["k"], inp["v"], inp["dO"], inp["valid"], inp["keep"]
    s, P, lse = _softmax(q, k, valid, scale)
    kd = keep.to(F64) * _drop_scale(p) if p else torch.ones_like(P)
    Pt = P * kd
    ctx = Pt @ v
    dV = Pt.transpose(-1, -2) @ dO
    dP = kd * (dO @ v.transpose(-1, -2))
    delta = (dO * ctx).sum(-1, keepdim=True)
    dS = P * (dP - delta) * scale
    return dict(s=s, lse=lse, P=P, Pt=Pt, ctx=ctx, dV=dV, dP=dP, delta=delta, dS=dS, dQ=dS @ k, dK=dS.transpose(-1, -2) @ q)


# ---- bars ------------------------------------------------------------------------------------------------------------------------
def lse_unit(inp, ref, scale):
    """2^-24 (scale max_k sum_d |q_d k_d| + |lse| + 1) per row, the maximum over the attended keys: K_LSE times this is the lse bar."""
    aqk = (inp["q"].abs() @ inp["k"].abs().transpose(-1, -2)) * scale
    aqk = aqk.masked_fill(~inp["valid"][:, None, None, :], 0.0)
    return U32 * (aqk.max(-1).values + ref["lse"].abs() + 1.0)


def bars(inp, ref, scale, readout=False, chained=False):
    """Allowances A per output, from the float64 reference alone.
    readout: V (dO) is an identity window, so ctx (dV) IS a window of P~ (P~^T): one bf16 rounding of the value itself, which the ulp term
    covers; only the fp32 terms of the probability (K_EXP) remain in A.
    chained: the backward is fed the forward kernel's own ctx and lse, whose errors are bounded by their bars instead of one rounding."""
    q, k, v, dO = inp["q"], inp["k"], inp["v"], inp["dO"]
    P, Pt, dS, ctx = ref["P"], ref["Pt"], ref["dS"], ref["ctx"]
    T = lambda x: x.transpose(-1, -2)
    unit = lse_unit(inp, ref, scale)
    aqk = (q.abs() @ T(k.abs())) * scale
    fp32 = K_EXP * U32 * (aqk + ref["lse"].abs()[..., None] + 1.0)        # relative fp32 error of one probability
    if readout:
        A_ctx = (Pt * fp32) @ v.abs()
        A_dV = T(Pt * fp32) @ dO.abs()
    else:
        A_ctx = U * (Pt @ v.abs())             # U: P~ is rounded to bf16 (2^-9) before P~ V, spare 2^-9 for fp32 / exp
        A_dV = U * (T(Pt) @ dO.abs())          # U: P~ is rounded to bf16 before P~^T dO
    # delta is formed from the bf16-rounded context the backward is given: |error of delta| <= eps
    ctx_err = HALF * ctx.abs() if not chained else bf16_ulp(_rb(ctx)) + A_ctx
    eps = (dO.abs() * ctx_err).sum(-1, keepdim=True)
    e = U * dS.abs() + 2 * scale * P * eps     # U: dS is rounded to bf16 before dS K and dS^T Q; the second term is delta's error in dS
    if chained:                                # ... and P = exp(s - lse) carries the forward's lse error as a relative one
        e = e + (K_LSE * unit)[..., None] * dS.abs()
    return dict(ctx=A_ctx, dV=A_dV, dQ=e @ k.abs(), dK=T(e) @ q.abs(), lse=K_LSE * unit, lse_unit=unit)


def check_bf16(got, ref64, A, rows=None):
    """got (float64 holding bf16 values) against ref64: (worst |got - bf16(ref)| / (ulp + A), share of elements further than one plain
    ulp from bf16(ref), i.e. those that need the allowance).  rows [B, S]: the rows that exist."""
    refb = _rb(ref64)
    diff = (got - refb).abs()
    ulp = bf16_ulp(refb)
    ratio = diff / (ulp + A)
    need = (diff > ulp).double()
    if rows is not None:
        sel = rows[:, None, :, None].expand_as(ratio)
        ratio, need = ratio[sel], need[sel]
    if not torch.isfinite(got if rows is None else got[sel]).all():
        return float("inf"), 1.0
    return ratio.max().item(), need.mean().item()


def check_lse(got, ref, unit, rows=None):
    """worst |got - lse| / (2^-24 (...)), i.e. the ratio at K_LSE = 1."""
    r = (got - ref["lse"]).abs() / unit
    if rows is not None:
        r = r[rows[:, None, :].expand_as(r)]
    return r.max().item() if torch.isfinite(r).all() else float("inf")


def check_all(case, inp, ref, A, out):
    """{output: (worst ratio, share needing the allowance)} for whatever of ctx, lse, dQ, dK, dV `out` holds."""
    res = {}
    for name in ("ctx", "dQ", "dK", "dV"):
        if name in out:
            res[name] = check_bf16(out[name], ref[name], A[name], inp["rows"])
    if "lse" in out:
        res["lse"] = (check_lse(out["lse"], ref, A["lse_unit"], inp["rows"]) / K_LSE, 0.0)
    return res


# ---- emulation of the kernels' arithmetic, and mutations of it -------------------------------------------------------------------
MUTATIONS = ("drop_key", "swap_v", "mask_shift", "ds_tile_unscaled", "ds_tile_2pct", "no_delta", "ragged_block", "lse_off")
TILE_LOCAL = ("ds_tile_unscaled", "ragged_block")        # caught in EVERY case that has the tile (a backward / any rows)
# ds_tile_2pct is the smallest of them: 2 % is ten roundings of dS, and it must leave a bar in every flat case that has the tile (where the
# keys are unit normal; a ramp or an offset in K widens A_dQ with |K| and a 2 % error of one tile no longer stands out of it)


def emulate(case, inp, ref, mut=None):
    """float64 with the kernels' two rounding points (P~ and dS to bf16 before the second products, outputs to bf16).  The backward is
    fed bf16(ctx_ref) and fp32(lse_ref), like the GPU tests.  mut: one of MUTATIONS, applied to sequence 0, head 0."""
    scale, p = case.scale, case.p
    q, k, v, dO, keep = inp["q"], inp["k"], inp["v"], inp["dO"], inp["keep"]
    valid = inp["valid"]
    T = lambda x: x.transpose(-1, -2)
    if mut == "mask_shift":
        valid = torch.roll(valid, 1, dims=-1)
    s, P, lse = _softmax(q, k, valid, scale)
    kd = keep.to(F64) * _drop_scale(p) if p else torch.ones_like(P)
    Pf = _rb(P * kd)                                           # rounding point 1 (forward)
    vf = v
    colmass = (ref["Pt"][0, 0] * inp["rows"][0][:, None]).sum(0)
    if mut == "drop_key":                                      # the key that carries most probability is left out of P V
        Pf = Pf.clone()
        Pf[0, 0, :, int(colmass.argmax())] = 0.0
    if mut == "swap_v":                                        # two adjacent keys' V rows exchanged
        j = int((colmass[:-1] + colmass[1:]).argmax()) if case.S > 1 else 0
        vf = v.clone()
        if case.S > 1:
            vf[0, 0, [j, j + 1]] = v[0, 0, [j + 1, j]]
    out = dict(ctx=_rb(Pf @ vf), lse=lse.clone())
    if mut == "lse_off":
        out["lse"][0, 0, 0] += 1e-3
    if case.has_bwd:
        ctx_in = _rb(ref["ctx"])
        lse_in = ref["lse"].to(torch.float32).to(F64)
        Pb = torch.exp(s - lse_in[..., None])
        delta = (dO * ctx_in).sum(-1, keepdim=True)
        if mut == "no_delta":
            delta = delta.clone()
            delta[0, 0] = 0.0
        dS = Pb * (kd * (dO @ T(v)) - delta) * scale
        if mut in ("ds_tile_unscaled", "ds_tile_2pct"):        # the 16-key tile that holds most of |dS|: `scale` forgotten / 2 % off
            t = int(ref["dS"][0, 0].abs().sum(0).unfold(0, min(16, case.S), min(16, case.S)).sum(-1).argmax()) * 16
            dS = dS.clone()
            dS[0, 0, :, t:t + 16] *= 1.02 if mut == "ds_tile_2pct" else 1.0 / scale
        dSr = _rb(dS)                                          # rounding point 1 (backward): dS, and P~ for dV
        out.update(dQ=_rb(dSr @ k), dK=_rb(T(dSr) @ q), dV=_rb(T(_rb(Pb * kd)) @ dO))
    if mut == "ragged_block":                                  # the last 16-row block of sequence 0 is never written
        n = int(inp["rows"][0].sum())
        for name in ("ctx", "dQ", "dK", "dV"):
            if name in out:
                out[name][0, :, 16 * ((n - 1) // 16):n] = 0.0
    return out


@functools.lru_cache(maxsize=4)
def prepared(case):
    """(inputs, float64 reference, bars) of a case, computed once and shared (callers must not modify them)."""
    inp = make_inputs(case)
    ref = reference(inp, case.scale, case.p)
    return inp, ref, bars(inp, ref, case.scale, readout=case.regime == "readout")
