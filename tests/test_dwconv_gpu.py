"""The depthwise 7x7 kernels of csrc/dwconv7.hip and csrc/dwconv7_mfma.hip (seventeen template instantiations behind mmg_dwconv7_nhwc,
mmg_dwconv7_nhwc_mfma and mmg_dwconv7_wgrad) against the float64 reference of tests/dwconv_ref.py; tests/test_dwconv_ref_cpu.py shows
on the CPU that the table reaches every instantiation, that a bar of zero is justified where it is used and that subtly wrong index
arithmetic leaves every bar.

Every case of dwconv_ref.CASES sets its knobs through the environment and runs ONE launch through the wrappers of mmgclip.kernels (which
read MMG_DWCONV_MFMA).  Integer and read-out cases: torch.equal against the reference cast to the output type.  Gaussian cases: the
derived bar (forward / data gradient) and the measured K_DW (weight gradient); every figure goes to `measured`.  Beside the numbers:
the launch is the instantiation dwconv_ref.instantiations names (mmg_last_kernel), the output buffer is pre-filled with NaN bits and
the rows past its end keep their sentinel, the item-loop cases assert the items per stream / workgroup they were built for.

What these tests found: the matrix-core kernel with the residual operand rounded TWICE - phase D packed conv + bias to bf16 for the
LDS transposes, phase F added the operand in fp32 and rounded again - where the VALU kernels add in fp32 and round once.  On the
parent's kernel conv-3x37x50x96-gaussian-mfma-flip-add-bias missed the bar by a factor of 218 (30 % of the elements differed from
bf16(ref), against 0.002 % without the operand), exactly what the CPU mutation pre_add_round of the emulation gives.  The ADD
instantiations now carry both halves of the fp32 accumulators to phase F (csrc/dwconv7_mfma.hip)."""
import pytest
import torch

from tests import dwconv_ref as R
from tests.conftest import measured

pytestmark = pytest.mark.gpu
BF, F64 = R.BF, R.F64
NAME = "dwconv_f64_"
OUT_FILL = 0x7FC1       # bf16 NaN bits in every output buffer: an unwritten pixel shows up as NaN
TAIL_FILL = 0x5A5A      # sentinel bits of the rows past the end of every buffer
EXTRA = 64              # pixels past the last one


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


def _dev_bf16(t, dev, tail=TAIL_FILL):
    """[n, H, W, C] float64 -> [n H W + EXTRA, C] bf16 on the device, sentinel bits in the extra rows."""
    C = t.shape[-1]
    buf = torch.full((t.numel() // C + EXTRA, C), tail, dtype=torch.int16).view(BF)
    buf[:t.numel() // C] = t.reshape(-1, C).to(torch.float32).to(BF)
    return buf.to(dev)


def _noted(fn):
    """Run one launch with the kernel notes on -> (result, mmg_last_kernel())."""
    from mmgclip import _hip
    lib = _hip.load()
    lib.mmg_set_kernel_notes(1)
    try:
        r = fn()
        name = lib.mmg_last_kernel().decode()
    finally:
        lib.mmg_set_kernel_notes(0)
    _sync()
    return r, name


def _conv(case, d, dev):
    """One forward / data-gradient launch -> (y [n, H, W, C] float64, the tail rows untouched, the kernel noted)."""
    from mmgclip import kernels as Kn
    n, H, W, C = case.n, case.H, case.W, case.C
    px = n * H * W
    x = _dev_bf16(d["x"], dev)
    w49 = d.get("w49_f32", d["w49"]).to(torch.float32).contiguous().to(dev)
    bias = None if d["bias"] is None else d["bias"].to(torch.float32).to(dev)
    add = None if d["add"] is None else _dev_bf16(d["add"], dev)
    out = torch.full((px + EXTRA, C), OUT_FILL, dtype=torch.int16).view(BF)
    out[px:] = torch.full((EXTRA, C), TAIL_FILL, dtype=torch.int16).view(BF)
    out = out.to(dev)
    _, name = _noted(lambda: Kn.dwconv7(x[:px], w49, bias, n, H, W, C, add=None if add is None else add[:px], flip=case.flip, out=out[:px]))
    host = out.cpu()
    tail_ok = bool((host[px:].view(torch.int16) == TAIL_FILL).all())
    return host[:px].to(F64).reshape(n, H, W, C), tail_ok, name


def _wgrad(case, d, dev):
    """One weight-gradient launch into pre-filled accumulators -> (dw [49, C], dbias [C] or None (float64), the kernel noted)."""
    from mmgclip import kernels as Kn
    n, H, W, C = case.n, case.H, case.W, case.C
    px = n * H * W
    x, dy = _dev_bf16(d["x"], dev), _dev_bf16(d["dy"], dev)
    fw, fb = R.fills(case)
    dw = torch.full((49, C), fw, dtype=torch.float32, device=dev)
    db = torch.full((C,), fb, dtype=torch.float32, device=dev) if case.bias else None
    _, name = _noted(lambda: Kn.dwconv7_wgrad(x[:px], dy[:px], dw, db, n, H, W, C))
    return dw.cpu().to(F64), None if db is None else db.cpu().to(F64), name


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_kernels_against_float64(case, dev, monkeypatch):
    """Every row of the table: bit-exact in the integer and read-out regimes, inside the derived (K = 64) / measured (K_DW) bars in
    the gaussian one; the launch is the instantiation the table names; the item-loop cases get the items they were built for."""
    from mmgclip import _hip
    _set_env(monkeypatch, case.env)
    d, ref = R.prepared(case)
    cus = _hip.load().mmg_device_cu_count()
    bad = []
    if case.op == "conv":
        if case.mfma and (case.n, case.H, case.W, case.C) in ((5, 250, 270, 32), (3, 170, 180, 128)):
            plan = R.mfma_plan(case.n, case.H, case.W, case.C, cus)          # the launcher's formula at this device's CU count
            print(case.id, "items per stream", plan["min_items"], "-", plan["max_items"], "on", cus, "CUs")
            assert plan["min_items"] >= 5 and all(plan["per_img"] % s for s in plan["strides"]), (cus, plan)
        y, tail_ok, name = _conv(case, d, dev)
        worst, differ = R.check_conv(case, ref, y)
        print(case.id, dict(worst=worst, differ_from_bf16_ref=differ, kernel=name))
        measured(NAME + case.id, worst=worst, differ_from_bf16_ref=differ, kernel=name)
        if not tail_ok:
            bad.append("rows past the end of y were written")
        if not torch.isfinite(y).all():
            bad.append(f"{int((~torch.isfinite(y)).sum())} elements of y unwritten (NaN fill) or not finite")
        if not worst <= 1.0:
            bad.append(f"y: worst ratio {worst} > 1 ({differ:.4f} of the elements differ from bf16(ref))")
    else:
        plan = R.wgrad_plan(case)
        if (case.n, case.H, case.W) in ((12, 9, 97), (48, 17, 9), (12, 9, 33)):
            print(case.id, "items per workgroup", plan["min_items"], "-", plan["max_items"])
            assert plan["min_items"] >= (1 if case.gth == 16 and case.H == 9 else 3) and plan["max_items"] >= 2, plan
        dw, db, name = _wgrad(case, d, dev)
        res = R.check_wgrad(case, ref, dw, db)
        vals = {k + "_ratio": v for k, v in res.items()}
        if case.regime == "gaussian":
            vals.update({k + "_ratio_k1": v * R.K_DW for k, v in res.items()})
        print(case.id, vals, name)
        measured(NAME + case.id, kernel=name, **vals)
        bad += [f"{k}: worst ratio {v} > 1" for k, v in res.items() if not v <= 1.0]
    if name != R.kernel_note(case):
        bad.append(f"launched {name!r}, the table says {R.kernel_note(case)!r}")
    planned = _hip.load().mmg_dwconv7_plan(*R.plan_args(case, 0)).decode().split(" grid=")[0]      # cus = 0: this device's
    if planned != name:
        bad.append(f"launched {name!r}, mmg_dwconv7_plan names {planned!r}")
    assert not bad, bad


SEAMS = [(1, 1, 1, 32), (2, 3, 5, 64), (1, 7, 7, 96), (2, 8, 32, 32), (1, 9, 33, 64), (2, 16, 32, 32), (1, 17, 33, 32)]


@pytest.mark.parametrize("shape", SEAMS, ids=lambda s: "x".join(map(str, s)))
def test_valu_kernels_give_the_same_bits_for_every_row_blocking_and_tile_height(shape, dev, monkeypatch):
    """One / two output rows per lane, 8- / 16-row tiles: every output accumulates its 49 taps in the same (kh, kw) order, so the
    forward (with bias) and the data gradient (flipped, with the residual operand) of gaussian data give identical bits - here on
    the degenerate maps and the exact-tile / one-pixel-over shapes."""
    for flip in (False, True):
        case = R.Case(*shape, "gaussian", "conv", 0, flip=flip, add=flip, bias=not flip)
        d = R.make_data(case)
        first = None
        for rows2, th in ((0, None), (1, 8), (1, 16)):
            c = case._replace(rows2=rows2, th=th)
            _set_env(monkeypatch, c.env)
            y, tail_ok, name = _conv(c, d, dev)
            assert tail_ok and torch.isfinite(y).all() and name == R.kernel_note(c), (name, rows2, th)
            first = y if first is None else first
            assert torch.equal(y, first), (flip, rows2, th)


@pytest.mark.parametrize("shape,waves", [((3, 37, 50, 96), None), ((9, 20, 35, 32), 8), ((1, 64, 70, 32), None)],
                         ids=["3x37x50x96", "9x20x35x32-w8", "1x64x70x32"])
def test_matrix_core_kernel_gives_the_same_bits_run_to_run(shape, waves, dev, monkeypatch):
    """Nothing in dwconv7_mfma_kernel depends on when a workgroup runs (no atomics; every LDS hand-over is behind a barrier): the
    data gradient with the residual operand on gaussian data, three times."""
    case = R.Case(*shape, "gaussian", "conv", 1, waves=waves, flip=True, add=True, bias=True)
    _set_env(monkeypatch, case.env)
    d = R.make_data(case)
    runs = [_conv(case, d, dev) for _ in range(3)]
    assert all(ok and torch.isfinite(y).all() for y, ok, _ in runs)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][0], runs[2][0])
