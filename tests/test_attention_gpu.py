"""The attention kernels of csrc/attention.hip (nine entry points) against the float64 reference of tests/attention_ref.py, with the
error bars derived there from the reference alone; tests/test_attention_ref_cpu.py shows on the CPU that those bars hold for the
kernels' arithmetic and that subtly wrong arithmetic leaves them.

Every case of attention_ref.CASES runs its forward and (where the family has one at that S) its backward through the C ABI
(mmgclip._hip.call), because the wrappers of mmgclip.kernels fix the scale and the leading dimensions.  The backward is fed
bf16(ctx_ref) and fp32(lse_ref), so that a forward error can neither hide nor cause a backward one; test_chained_* feed the forward
kernel's own outputs.  Beside the numbers: padding columns, rows past the packed total and lse past a packed sequence's length keep
their sentinel bits; dK and dV of masked keys are exactly zero; the tiled kernels give the same bits run to run and for every
rows-per-wave setting."""
import pytest
import torch

from tests import attention_ref as R
from tests.conftest import measured

pytestmark = pytest.mark.gpu
BF, F64 = R.BF, R.F64
NAME = "test_attention_gpu."
IN_FILL = 0x7FC1        # bf16 NaN in the padding of every input: a stray read shows up as NaN
OUT_FILL = 0x5A5A       # sentinel bits of every output buffer
LSE_FILL = 12345.0
EXTRA = 2               # rows past the last one of every buffer (packed layout: past cu_seqlens[B])
FWD = {"whole": "mmg_attention_fwd", "tiled": "mmg_attention_long_fwd", "packed": "mmg_attention_varlen_fwd",
       "drop": "mmg_attention_dropout_fwd", "drop_packed": "mmg_attention_dropout_fwd"}


def _hip():
    from mmgclip import _hip
    return _hip


def _lds(case):
    """(ld, ldc, lddc, lddq): the minimum, or each wider by a different multiple of 8."""
    Hd = case.heads * 64
    return (3 * Hd + 8, Hd + 16, Hd + 24, 3 * Hd + 40) if case.wide else (3 * Hd, Hd, Hd, 3 * Hd)


def _to_rows(t, case):
    """[B, heads, S, 64] -> [rows, heads * 64] bf16 in the case's layout."""
    B, H, S = case.B, case.heads, case.S
    x = t.permute(0, 2, 1, 3).reshape(B, S, H * 64).to(torch.float32).to(BF)
    return torch.cat([x[b, :n] for b, n in enumerate(case.lens)]) if case.lens else x.reshape(B * S, H * 64)


def _from_rows(m, case):
    """Inverse of _to_rows, float64 (rows a packed sequence does not have: zero)."""
    B, H, S = case.B, case.heads, case.S
    if case.lens:
        x, r = torch.zeros(B, S, H * 64, dtype=BF), 0
        for b, n in enumerate(case.lens):
            x[b, :n] = m[r:r + n]
            r += n
    else:
        x = m.reshape(B, S, H * 64)
    return x.reshape(B, S, H, 64).permute(0, 2, 1, 3).to(F64)


def _buffer(data, ld, fill, dev):
    """[rows + EXTRA, ld] bf16 on the device: data, and `fill` bits in the padding columns and the extra rows."""
    rows, width = data.shape
    buf = torch.full((rows + EXTRA, ld), fill, dtype=torch.int16).view(BF)
    buf[:rows, :width] = data
    return buf.to(dev)


def _out_buffer(rows, ld, dev):
    return torch.full((rows + EXTRA, ld), OUT_FILL, dtype=torch.int16).view(BF).to(dev)


def _untouched(buf, rows, width):
    """The padding columns and the extra rows of an output buffer still hold the sentinel bits."""
    b = buf.cpu().view(torch.int16)
    return bool((b[:, width:] == OUT_FILL).all() and (b[rows:] == OUT_FILL).all())


class _Run:
    """The device operands of one case: qkv, mask / cu_seqlens, the dropout arguments."""

    def __init__(self, case, inp, dev, family=None):
        h = _hip()
        self.case, self.inp, self.dev, self.family = case, inp, dev, family or case.family
        self.B, self.S, self.H, self.Hd = case.B, case.S, case.heads, case.heads * 64
        self.ld, self.ldc, self.lddc, self.lddq = _lds(case)
        qkv = torch.cat([_to_rows(inp[n], case) for n in "qkv"], dim=1)
        self.rows = qkv.shape[0]
        self.qkv = _buffer(qkv, self.ld, IN_FILL, dev)
        self.mask = None if case.mask == "none" or case.lens else inp["valid"].long().to(dev)
        self.cu = None
        if case.lens:
            self.cu = torch.tensor([0] + torch.tensor(case.lens).cumsum(0).tolist(), dtype=torch.int32).to(dev)
        self.ptr, self.call, self.stream = h.ptr, h.call, h.stream
        self.dims = (self.B, self.S, self.H, self.Hd, float(case.scale))
        self.drop = (float(case.p), R.SEED, R.SITE, 0)

    def forward(self, p=None):
        """-> ctx [B, heads, S, 64] float64, lse [B, heads, S] float64, (ctx buffer, lse tensor)."""
        f, ptr = self.family, self.ptr
        ctx = _out_buffer(self.rows, self.ldc, self.dev)
        lse = torch.full((self.B, self.H, self.S), LSE_FILL, dtype=torch.float32, device=self.dev)
        if f in ("whole", "tiled"):
            self.call(FWD[f], ptr(self.qkv), self.ld, ptr(self.mask), ptr(ctx), self.ldc, ptr(lse), *self.dims, self.stream())
        elif f == "packed":
            self.call(FWD[f], ptr(self.qkv), self.ld, ptr(self.cu), ptr(ctx), self.ldc, ptr(lse), *self.dims, self.stream())
        else:
            drop = self.drop if p is None else (float(p),) + self.drop[1:]
            self.call(FWD[f], ptr(self.qkv), self.ld, ptr(self.mask), ptr(self.cu), ptr(ctx), self.ldc, ptr(lse), *self.dims, *drop,
                      self.stream())
        torch.cuda.synchronize()
        return _from_rows(ctx.cpu()[:self.rows, :self.Hd], self.case), lse.cpu().to(F64), (ctx, lse)

    def backward(self, ctx_in, lse_in, p=None):
        """ctx_in [B, heads, S, 64] (bf16-exact float64), lse_in [B, heads, S] -> dQ, dK, dV float64, dqkv buffer."""
        f, ptr, case = self.family, self.ptr, self.case
        ctx = _buffer(_to_rows(ctx_in, case), self.ldc, IN_FILL, self.dev)
        dctx = _buffer(_to_rows(self.inp["dO"], case), self.lddc, IN_FILL, self.dev)
        lse = lse_in.to(torch.float32).to(self.dev).contiguous()
        dqkv = _out_buffer(self.rows, self.lddq, self.dev)
        ws = torch.empty(self.B * self.H * self.S, dtype=torch.float32, device=self.dev)
        ops = (ptr(ctx), self.ldc, ptr(lse), ptr(dctx), self.lddc, ptr(dqkv), self.lddq)
        drop = self.drop if p is None else (float(p),) + self.drop[1:]
        if f == "whole":
            self.call("mmg_attention_bwd", ptr(self.qkv), self.ld, ptr(self.mask), *ops, *self.dims, self.stream())
        elif f == "tiled":
            self.call("mmg_attention_long_bwd", ptr(self.qkv), self.ld, ptr(self.mask), *ops, ptr(ws), *self.dims, self.stream())
        elif f == "packed":
            self.call("mmg_attention_varlen_bwd", ptr(self.qkv), self.ld, ptr(self.cu), *ops, *self.dims, self.stream())
        elif self.S > 256:
            self.call("mmg_attention_dropout_long_bwd", ptr(self.qkv), self.ld, ptr(self.mask), *ops, ptr(ws), *self.dims, *drop,
                      self.stream())
        else:
            self.call("mmg_attention_dropout_bwd", ptr(self.qkv), self.ld, ptr(self.mask), ptr(self.cu), *ops, *self.dims, *drop,
                      self.stream())
        torch.cuda.synchronize()
        g = dqkv.cpu()[:self.rows]
        dq, dk, dv = [_from_rows(g[:, i * self.Hd:(i + 1) * self.Hd].contiguous(), case) for i in range(3)]
        return dict(dQ=dq, dK=dk, dV=dv), dqkv


def _set_rb(monkeypatch, rb, rbk):
    for name, v in (("MMG_ATT_RB", rb), ("MMG_ATT_RB_DKV", rbk)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)


def _report(name, res):
    """Print and record every figure (worst ratio and share needing the allowance per output; the lse ratio at K_LSE = 1)."""
    vals = {}
    for out, (worst, share) in res.items():
        if out == "lse":
            vals["lse_ratio"] = worst
            vals["lse_ratio_k1"] = worst * R.K_LSE
        else:
            vals[out + "_worst"] = worst
            vals[out + "_need_allowance"] = share
    print(name, vals)
    measured(NAME + name, **vals)


def _check_case(case, run, inp, ref, A, tag=""):
    """Forward and backward of one case on one kernel family; returns the failures as a list of strings."""
    ctx, lse, (ctx_buf, lse_buf) = run.forward()
    out = dict(ctx=ctx, lse=lse)
    bad = []
    if not _untouched(ctx_buf, run.rows, run.Hd):
        bad.append("ctx padding / extra rows were written")
    if case.lens:                                        # lse past a packed sequence's length is not written
        raw = lse_buf.cpu()
        if not all(bool((raw[b, :, n:] == LSE_FILL).all()) for b, n in enumerate(case.lens)):
            bad.append("lse past a packed sequence's length was written")
    if run.family in ("tiled", "drop") or case.S <= 256:
        grads, dqkv = run.backward(R._rb(ref["ctx"]), ref["lse"])
        out.update(grads)
        if not _untouched(dqkv, run.rows, 3 * run.Hd):
            bad.append("dqkv padding / extra rows were written")
        dead = (~inp["valid"] & inp["rows"])[:, None, :, None]              # masked keys of the padded layout
        for n in ("dK", "dV"):
            if not bool((grads[n] * dead == 0).all()):
                bad.append(f"{n} of a masked key is not exactly zero")
    res = R.check_all(case, inp, ref, A, out)
    _report(case.id + tag, res)
    bad += [f"{k}: worst ratio {w:.3f} > 1" for k, (w, _) in res.items() if not w <= 1.0]
    return bad


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_kernels_against_float64(case, dev, monkeypatch):
    """ctx, lse, dQ, dK, dV of every table row inside the bars of attention_ref.bars.  A tiled case whose S the whole-sequence kernels
    accept too runs on them as well: both against the float64 reference, not against each other."""
    _set_rb(monkeypatch, case.rb, case.rbk)
    inp, ref, A = R.prepared(case)
    bad = _check_case(case, _Run(case, inp, dev), inp, ref, A)
    if case.family == "tiled" and case.S <= 512:
        bad += ["whole-sequence kernels: " + b for b in _check_case(case, _Run(case, inp, dev, family="whole"), inp, ref, A, "/whole")]
    assert not bad, bad


CHAINED = [c for c in R.CASES if c.id in (
    "whole-S97-flat-right-bh2x2", "packed-S77-flat-none-bh3x2", "tiled-S130-flat-left-bh2x2-rb22", "drop-S97-flat-right-bh2x2-drop",
    "drop-S257-flat-right-bh2x2-drop")]


@pytest.mark.parametrize("case", CHAINED, ids=lambda c: c.id)
def test_chained_backward_from_the_forward_kernels_own_outputs(case, dev, monkeypatch):
    """One case per family: the backward is fed the ctx and lse the forward kernel wrote.  Their errors are bounded by the forward's
    bars, which attention_ref.bars(chained=True) puts in the place of the single rounding of bf16(ctx_ref)."""
    assert len(CHAINED) == 5
    _set_rb(monkeypatch, case.rb, case.rbk)
    inp, ref, _ = R.prepared(case)
    A = R.bars(inp, ref, case.scale, chained=True)
    run = _Run(case, inp, dev)
    ctx, lse, _ = run.forward()
    grads, _ = run.backward(ctx, lse)
    res = R.check_all(case, inp, ref, A, grads)
    _report(case.id + "/chained", res)
    assert all(w <= 1.0 for w, _ in res.values()), res


@pytest.mark.parametrize("S", [97, 257])
def test_dropout_with_p_zero_is_the_plain_kernel_bit_for_bit(dev, monkeypatch, S):
    """p = 0 keeps everything at scale 1: the DROP instantiations must reproduce the plain ones' bits (S = 257: the tiled DROP
    backward, which runs two row blocks per wave, against the plain tiled backward at that setting)."""
    _set_rb(monkeypatch, 2, 2)
    case = next(c for c in R.CASES if c.family == "drop" and c.S == S and c.regime == "flat" and not c.wide)
    inp, ref, _ = R.prepared(case)
    drop, plain = _Run(case, inp, dev), _Run(case, inp, dev, family="whole")
    ctx_d, lse_d, _ = drop.forward(p=0.0)
    ctx_p, lse_p, _ = plain.forward()
    assert torch.equal(ctx_d, ctx_p) and torch.equal(lse_d, lse_p)
    if S > 256:
        plain = _Run(case, inp, dev, family="tiled")
    g_d, _ = drop.backward(ctx_p, lse_p, p=0.0)
    g_p, _ = plain.backward(ctx_p, lse_p)
    for n in ("dQ", "dK", "dV"):
        assert torch.equal(g_d[n], g_p[n]), n


@pytest.mark.parametrize("mask", ["none", "holes"])
def test_tiled_kernels_give_the_same_bits_run_to_run_and_for_every_rows_per_wave(dev, monkeypatch, mask):
    """S = 300 with B x heads = 8.  A row's arithmetic does not depend on how many row blocks a wave owns, nor on when its workgroup
    runs: the tiled forward twice in a row, then MMG_ATT_RB = 1, 2, 4 (forward and dQ) and MMG_ATT_RB_DKV = 1, 2, 3 (dK, dV), must all
    give the same bits.  (The property tools/att_check.py checks by hand at S = 4097: a tile read before its LDS-DMA had landed
    showed up as rounding-size differences between launches.)"""
    case = R.Case("tiled", 300, "flat", mask, heads=4)
    inp = R.make_inputs(case)
    ref = R.reference(inp, case.scale)
    run = _Run(case, inp, dev)
    first = None
    for rb, rbk in ((1, 1), (1, 1), (2, 2), (4, 3)):
        _set_rb(monkeypatch, rb, rbk)
        ctx, lse, _ = run.forward()
        grads, _ = run.backward(R._rb(ref["ctx"]), ref["lse"])
        got = dict(ctx=ctx, lse=lse, **grads)
        assert all(torch.isfinite(t).all() for t in got.values())
        if first is None:
            first = got
        for n, t in got.items():
            assert torch.equal(t, first[n]), (n, rb, rbk)
