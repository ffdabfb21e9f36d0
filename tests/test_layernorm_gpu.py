"""The LayerNorm kernels of csrc/norm_elementwise.hip (28 template instantiations behind mmg_layernorm_fwd, mmg_layernorm_fwd_f32,
mmg_layernorm_fwd_fp8, mmg_layernorm_bwd and mmg_layernorm_bwd_f32) against the float64 reference of tests/layernorm_ref.py;
tests/test_layernorm_ref_cpu.py shows on the CPU that the table reaches every instantiation and call mode, that torch.equal is justified
where it is used and that subtly wrong arithmetic leaves every bar.

Every case of layernorm_ref.CASES sets MMG_LN_PLAIN / MMG_LN_CH3 through the environment (ln_knobs reads them per call) and runs ONE
launch through mmgclip._hip.call on buffers of the test's own: every output - mean and rstd too - is pre-filled with NaN bits and
carries sentinel rows past the last row the kernel owns (patchified outputs: past row n (H/2) (W/2)) and, where its leading dimension is
wider than its row, sentinel columns; strided inputs carry NaN in the columns no kernel may read.  Integer cases: torch.equal against
the reference cast to the output type for the outputs layernorm_ref lists as exact.  Everything else: the derived bars; every figure
goes to `measured`.  Beside the numbers: the launch is the instantiation the table names and the one mmg_layernorm_plan names for the
same call (mmg_last_kernel; the plan itself is pinned on the CPU, tests/test_layernorm_plan_cpu.py), no owned element holds a NaN
fill, every sentinel is intact, rows that are equal (the rows have period P) give equal bits - the large cases (grid-stride loop,
non-temporal stores) are compared on the device against the P reference rows gathered by row % P -, dgamma / dbeta start from a non-zero
pre-fill, y = bf16(yf) and x_after = fp32(x + res) bit for bit.

What these tests found: no wrong result.  On the first MI355X run every integer case was bit-exact, every kernel note matched and every
gaussian figure was inside its derived bar with K_RSQ = 1 (worst rstd ratio 0.128).  One host-side change came with the tests
(csrc/norm_elementwise.hip): MMG_LN_PLAIN and MMG_LN_CH3 are read per call.  DESIGN.md, "LayerNorm kernels against float64"."""
import ctypes

import pytest
import torch

from mmgclip import _hip
from tests import layernorm_ref as R
from tests.conftest import measured

pytestmark = pytest.mark.gpu
BF, F64, F32 = R.BF, R.F64, R.F32
NAME = "layernorm_f64_"
EXTRA = 64                                                 # sentinel rows: a whole block of the narrowest kernel
# (int dtype, NaN bits of the owned elements, sentinel bits)
KINDS = {"bf16": (torch.int16, 0x7FC1, 0x5A5A), "f32": (torch.int32, 0x7FC00001, 0x5A5A5A5A), "fp8": (torch.uint8, 0x7F, 0x5A)}
VIEW = {"bf16": BF, "f32": F32, "fp8": torch.uint8}


def _sync():
    """A GPU fault ends the run: nothing more is started on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, stopping: {e}", returncode=3)


def _set_env(monkeypatch, env):
    for name, v in env.items():
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


class Buf:
    """[rows + EXTRA, ld] (cols = 0: [rows + EXTRA]) output: NaN bits in the rows x cols the kernel owns, sentinel bits elsewhere."""

    def __init__(self, kind, rows, cols, ld, dev):
        it, fill, tail = KINDS[kind]
        self.kind, self.rows, self.cols = kind, rows, cols
        self.raw = torch.full((rows + EXTRA, ld) if cols else (rows + EXTRA,), tail, dtype=it, device=dev)
        self.own = self.raw[:rows, :cols] if cols else self.raw[:rows]
        self.own.fill_(fill)
        self.t = self.raw.view(VIEW[kind])

    def load(self, values):
        """Input that is also an output (x of the fp32-row forward with res)."""
        self.body.copy_(values)

    @property
    def body(self):
        return self.t[:self.rows, :self.cols] if self.cols else self.t[:self.rows]

    def sentinels_ok(self):
        tail = KINDS[self.kind][2]
        ok = bool((self.raw[self.rows:] == tail).all())
        if self.cols and self.raw.shape[1] > self.cols:
            ok = ok and bool((self.raw[:self.rows, self.cols:] == tail).all())
        return ok

    def untouched(self):
        return bool((self.own == KINDS[self.kind][1]).all())

    def written(self):
        """No NaN fill (and nothing else that is not finite) is left in an owned element."""
        if self.kind == "fp8":
            return bool(((self.own & 0x7F) != 0x7F).all())
        return bool(torch.isfinite(self.body).all())


def _input(base, src, C, ld, dev, dtype):
    """Base rows [n, C] float64 -> the M periodic rows on the device, [M, ld]; the columns past C hold NaN."""
    rows = base.to(F32).to(dtype).to(dev)[src]
    if ld == C:
        return rows.contiguous()
    wide = torch.full((rows.shape[0], ld), float("nan"), dtype=dtype, device=dev)
    wide[:, :C] = rows
    return wide


def _f32(t, dev):
    return t.to(F32).contiguous().to(dev)


def _launch(case, d, dev):
    """The case's launch -> ({output: Buf}, {accumulated output: device tensor}, kernel noted, the call's arguments kept alive)."""
    call, ptr, stream = _hip.call, _hip.ptr, _hip.stream
    C, M = case.C, case.M
    n = R.base_rows(case)
    src = (torch.arange(M) % n).to(dev)
    ld = lambda name: C + case.pad if case.strided == name else C
    xt = F32 if case.x32 else BF
    gamma, beta = _f32(d["gamma"], dev), _f32(d["beta"], dev)
    eps = float(d["eps"])
    patch, (H, W) = int(bool(case.patch)), case.patch or (0, 0)
    prow = R.patch_rows(M, H, W) if case.patch else M
    pld = lambda name: (4 * C + case.pad if case.strided == name else 4 * C) if case.patch else ld(name)
    outs, accs, keep = {}, {}, []
    lib = _hip.load()
    if case.op == "fwd":
        if case.res:                                       # x is overwritten with x + res
            outs["x_after"] = Buf("f32", M, C, ld("x"), dev)
            outs["x_after"].load(d["x"].to(F32).to(dev)[src])
            x = outs["x_after"].t
        else:
            x = _input(d["x"], src, C, ld("x"), dev, xt)
        outs["y"] = Buf("fp8" if case.fp8 else "bf16", prow, 4 * C if case.patch else C, pld("y"), dev)
        if case.stats:
            outs.update(mean=Buf("f32", M, 0, 0, dev), rstd=Buf("f32", M, 0, 0, dev))
        g = lambda k: ptr(outs[k].t) if k in outs else None
        if case.fp8:
            fn = lambda: call("mmg_layernorm_fwd_fp8", ptr(x), ld("x"), ptr(gamma), ptr(beta), eps, g("y"), ld("y"), g("mean"), g("rstd"),
                              M, C, stream())
        elif case.x32:
            res = _input(d["res"], src, C, ld("res"), dev, F32) if case.res else None
            if case.yf:
                outs["yf"] = Buf("f32", M, C, ld("yf"), dev)
            keep.append(res)
            fn = lambda: call("mmg_layernorm_fwd_f32", ptr(x), ld("x"), ptr(res), ld("res") if case.res else 0, ptr(gamma), ptr(beta), eps,
                              g("y"), ld("y"), g("yf"), ld("yf") if case.yf else 0, g("mean"), g("rstd"), M, C, stream())
        else:
            fn = lambda: call("mmg_layernorm_fwd", ptr(x), ld("x"), ptr(gamma), ptr(beta), eps, g("y"), pld("y"), g("mean"), g("rstd"),
                              M, C, patch, H, W, stream())
    else:
        x = _input(d["xs"], src, C, ld("x"), dev, xt)
        mean, rstd = _f32(d["mean32"], dev)[src].contiguous(), _f32(d["rstd32"], dev)[src].contiguous()
        dy_rows = d["dy"].to(F32).to(BF).to(dev)[src]
        if case.patch:
            dy_rows = R.to_patch(dy_rows, H, W)
        dy = _input(dy_rows, torch.arange(dy_rows.shape[0], device=dev), dy_rows.shape[1], pld("dy"), dev, BF)
        add = _input(d["add"], src, C, ld("add"), dev, BF) if case.add else None
        outs["dx"] = Buf("bf16", M, C, ld("dx"), dev)
        if case.grads:
            accs = {k: torch.full((C,), R.FILL[k], dtype=F32, device=dev) for k in ("dgamma", "dbeta")}
        keep += [mean, rstd, dy, add]
        tail = (ptr(add), ld("add") if case.add else 0, stream())
        head = (ptr(dy), pld("dy"), ptr(x), ld("x"), ptr(mean), ptr(rstd), ptr(gamma), ptr(outs["dx"].t), ld("dx"), ptr(accs.get("dgamma")),
                ptr(accs.get("dbeta")), M, C)
        if case.x32:
            fn = lambda: call("mmg_layernorm_bwd_f32", *head, *tail)
        else:
            fn = lambda: call("mmg_layernorm_bwd", *head, patch, H, W, *tail)
    keep += [x, gamma, beta]
    _sync()
    lib.mmg_set_kernel_notes(1)
    try:
        fn()
        name = lib.mmg_last_kernel().decode()
    finally:
        lib.mmg_set_kernel_notes(0)
    _sync()
    return outs, accs, name, keep


def _run(case, dev, monkeypatch, d=None):
    _set_env(monkeypatch, case.env)
    if d is None:
        d = R.prepared(case)[0]
    return _launch(case, d, dev)


def _rows_of(case, name, buf):
    """The output in the row layout [M, C] (mean / rstd: [M]) as the reference holds it; fp8: the raw bytes."""
    if name == "y" and case.patch:
        return R.from_patch(buf.body, case.M, *case.patch)
    return buf.body


def _bits(t):
    return t.view({F32: torch.int32, BF: torch.int16, torch.uint8: torch.uint8}[t.dtype])


def _decode(case, name, t):
    """Device rows -> float64 on the CPU."""
    if name == "y" and case.fp8:
        return t.cpu().view(torch.float8_e4m3fn).to(F32).to(F64)
    return t.cpu().to(F64)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_kernels_against_float64(case, dev, monkeypatch):
    """Every row of the table: bit-exact where layernorm_ref.exact_outputs says so, inside the derived bars elsewhere; the launch is the
    instantiation the table names; sentinels, fills, equal rows and the exact relations as the module docstring lists them."""
    d, ref, bar, _ = R.prepared(case)
    outs, accs, name, _ = _run(case, dev, monkeypatch)
    M, n = case.M, R.base_rows(case)
    bad, vals = [], {}
    assert set(outs) | set(accs) == set(R.outputs_of(case)), (sorted(outs), sorted(accs))
    src = (torch.arange(M) % n).to(dev)
    for k, buf in outs.items():
        if not buf.sentinels_ok():
            bad.append(f"{k}: a sentinel row or column was written")
        if not buf.written():
            bad.append(f"{k}: owned elements unwritten (NaN fill) or not finite")
        rows = _rows_of(case, k, buf)
        if M > n and not torch.equal(_bits(rows), _bits(rows[:n])[src]):
            bad.append(f"{k}: equal rows gave different bits")
        worst, differ = R.check(case, k, _decode(case, k, rows[:n]), ref[k], bar[k])
        vals[k + "_ratio"], vals[k + "_differ"] = worst, differ
    for k, t in accs.items():
        worst, differ = R.check(case, k, t.cpu().to(F64), ref[k], bar[k])
        vals[k + "_ratio"], vals[k + "_differ"] = worst, differ
    if case.yf and not torch.equal(_bits(outs["y"].body), _bits(outs["yf"].body.to(BF))):
        bad.append("y is not bf16(yf) bit for bit")
    print(case.id, vals, name)
    measured(NAME + case.id, kernel=name, rows=M, k_rsq=R.K_RSQ, **vals)
    exact = R.exact_outputs(case)
    for k in list(outs) + list(accs):
        if not vals[k + "_ratio"] <= 1.0:
            bad.append(f"{k}: " + ("not bit-exact" if k in exact else f"worst ratio {vals[k + '_ratio']} > 1")
                       + f" ({vals[k + '_differ']:.5f} of the elements differ from the reference cast to the output type)")
    if name != R.kernel_note(case):
        bad.append(f"launched {name!r}, the table says {R.kernel_note(case)!r}")
    planned = _hip.load().mmg_layernorm_plan(*case.plan_args).decode().split(" grid=")[0]     # (monkeypatch still holds the case's knobs)
    if name != planned:
        bad.append(f"launched {name!r}, mmg_layernorm_plan names {planned!r}")
    assert not bad, bad


@pytest.mark.parametrize("C,plain", [(192, None), (384, 0), (256, None), (1024, None)])
@pytest.mark.parametrize("HW", [(4, 6), (5, 7)])
def test_patchified_y_is_a_permutation_of_the_plain_y(C, plain, HW, dev, monkeypatch):
    a = R.Case("fwd", C, 3 * HW[0] * HW[1], "gaussian", plain=plain)
    b = a._replace(patch=HW)
    assert R.instantiation(a) == R.instantiation(b)
    d = R.prepared(a)[0]
    ya = _run(a, dev, monkeypatch, d)[0]["y"]
    yb = _run(b, dev, monkeypatch, d)[0]["y"]
    live = R.patch_map(a.M, *HW)[0].to(dev)
    assert ya.written() and yb.written() and yb.sentinels_ok()
    assert torch.equal(_bits(R.from_patch(yb.body, a.M, *HW))[live], _bits(ya.body)[live])


@pytest.mark.parametrize("C,plain", [(256, None), (768, 0), (1032, None), (8, None)])
def test_fp32_row_kernel_on_bf16_exact_rows_gives_the_bf16_row_kernels_bits(C, plain, dev, monkeypatch):
    """Where both entry points run the same instantiation they differ in the load alone: y, mean and rstd are identical."""
    a = R.ragged(R.Case("fwd", C, 0, "gaussian", plain=plain))
    b = a._replace(x32=True)
    assert R.instantiation(a) == R.instantiation(b)
    d = R.prepared(a)[0]
    oa, _, na, _ = _run(a, dev, monkeypatch, d)
    ob, _, nb, _ = _run(b, dev, monkeypatch, d)
    assert na == nb == R.kernel_note(a)
    assert all(torch.equal(_bits(oa[k].body), _bits(ob[k].body)) for k in ("y", "mean", "rstd"))


@pytest.mark.parametrize("case", [R.ragged(R.Case("fwd", 384, 0, "gaussian")), R.ragged(R.Case("fwd", 1032, 0, "gaussian", x32=True, yf=True)),
                                  R.ragged(R.Case("bwd", 192, 0, "gaussian")), R.ragged(R.Case("bwd", 2056, 0, "gaussian", add=True))],
                         ids=lambda c: c.id)
def test_row_outputs_give_the_same_bits_run_to_run(case, dev, monkeypatch):
    """Nothing but dgamma / dbeta depends on when a block runs."""
    runs = [{k: _bits(v.body).clone() for k, v in _run(case, dev, monkeypatch)[0].items()} for _ in range(3)]
    assert all(torch.equal(runs[0][k], r[k]) for r in runs[1:] for k in runs[0])


REJECTED = {
    "C=4104": dict(C=4104), "C=12": dict(C=12), "ldx=C+4": dict(ldx=260), "patch, M % (H W) != 0": dict(patch=1, H=3, W=5, ldy=1024, lddy=1024),
    "ldy < 4C with patch": dict(patch=1, H=4, W=4, ldy=512, lddy=512), "dgamma without dbeta": dict(no_dbeta=True),
    "lddy < C": dict(lddy=128),
}


@pytest.mark.parametrize("what", list(REJECTED))
def test_bad_arguments_are_rejected_and_nothing_is_launched(what, dev):
    """An error string comes back, no kernel is noted and the outputs keep their fill."""
    lib, ptr = _hip.load(), _hip.ptr
    kw = dict(C=256, M=16, ldx=None, ldy=None, lddy=None, patch=0, H=0, W=0, no_dbeta=False)
    kw.update(REJECTED[what])
    C, M = kw["C"], kw["M"]
    ldx, ldy, lddy = kw["ldx"] or C, kw["ldy"] or C, kw["lddy"] or C
    wide = 4 * 4104 + 64                                   # every buffer holds the widest row any of these calls could name
    x = torch.zeros(M, wide, dtype=BF, device=dev)
    x32 = torch.zeros(M, wide, dtype=F32, device=dev)
    dy = torch.zeros(M, wide, dtype=BF, device=dev)
    gamma, beta = torch.ones(wide, dtype=F32, device=dev), torch.zeros(wide, dtype=F32, device=dev)
    stats = torch.ones(M + EXTRA, dtype=F32, device=dev)
    y, dx, yf = Buf("bf16", M, wide, wide, dev), Buf("bf16", M, wide, wide, dev), Buf("f32", M, wide, wide, dev)
    mean, rstd = Buf("f32", M, 0, 0, dev), Buf("f32", M, 0, 0, dev)
    dg, db = torch.full((wide,), 0.5, dtype=F32, device=dev), torch.full((wide,), -3.0, dtype=F32, device=dev)
    s = _hip.stream()
    eps = ctypes.c_float(1e-6)
    _sync()
    lib.mmg_set_kernel_notes(1)
    try:
        before = lib.mmg_last_kernel()
        calls = {}
        fwd_only = what == "ldy < 4C with patch"
        bwd_only = what in ("dgamma without dbeta", "lddy < C")
        if not bwd_only:
            calls["mmg_layernorm_fwd"] = lambda: lib.mmg_layernorm_fwd(ptr(x), ldx, ptr(gamma), ptr(beta), eps, ptr(y.t), ldy, ptr(mean.t),
                                                                       ptr(rstd.t), M, C, kw["patch"], kw["H"], kw["W"], s)
            if not kw["patch"]:
                calls["mmg_layernorm_fwd_f32"] = lambda: lib.mmg_layernorm_fwd_f32(ptr(x32), ldx, None, 0, ptr(gamma), ptr(beta), eps, ptr(y.t),
                                                                                   ldy, ptr(yf.t), ldy, ptr(mean.t), ptr(rstd.t), M, C, s)
                calls["mmg_layernorm_fwd_fp8"] = lambda: lib.mmg_layernorm_fwd_fp8(ptr(x), ldx, ptr(gamma), ptr(beta), eps, ptr(y.t), ldy,
                                                                                   ptr(mean.t), ptr(rstd.t), M, C, s)
        if not fwd_only:
            dbp = None if kw["no_dbeta"] else ptr(db)
            calls["mmg_layernorm_bwd"] = lambda: lib.mmg_layernorm_bwd(ptr(dy), lddy, ptr(x), ldx, ptr(stats), ptr(stats), ptr(gamma), ptr(dx.t),
                                                                       C, ptr(dg), dbp, M, C, kw["patch"], kw["H"], kw["W"], None, 0, s)
            if not kw["patch"]:
                calls["mmg_layernorm_bwd_f32"] = lambda: lib.mmg_layernorm_bwd_f32(ptr(dy), lddy, ptr(x32), ldx, ptr(stats), ptr(stats), ptr(gamma),
                                                                                   ptr(dx.t), C, ptr(dg), dbp, M, C, None, 0, s)
        for name, fn in calls.items():
            assert fn() != 0, (what, name)
            assert name in lib.mmg_last_error().decode(), (what, name, lib.mmg_last_error())
            assert lib.mmg_last_kernel() == before, (what, name)
    finally:
        lib.mmg_set_kernel_notes(0)
    _sync()
    assert all(b.untouched() and b.sentinels_ok() for b in (y, dx, yf, mean, rstd))
    assert bool((dg == 0.5).all()) and bool((db == -3.0).all())
