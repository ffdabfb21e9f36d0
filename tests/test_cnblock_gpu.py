"""The fused ConvNeXt block MLP kernels of csrc/cnblock_mlp.hip and csrc/cnblock_bwdw.hip (28 template instantiations behind
mmg_cnblock_mlp_fwd, mmg_cnblock_mlp_bwd and mmg_cnblock_bwdw) against the float64 reference of tests/cnblock_ref.py;
tests/test_cnblock_ref_cpu.py shows on the CPU that the table reaches every instantiation, that torch.equal is justified where it is
used and that subtly wrong arithmetic leaves every bar.

Every case of cnblock_ref.CASES sets its knobs through the environment and runs ONE launch of the entry point (cnblock_bwdw: the two
launches behind it) through mmgclip._hip.call on buffers of the test's own: every output is pre-filled with NaN bits and carries EXTRA
sentinel rows past row M.  Integer cases: torch.equal against the reference cast to the output type for the outputs cnblock_ref lists
as exact.  Everything else: the derived bars; every figure goes to `measured`.  Beside the numbers: the launch is the instantiation the
table names (mmg_last_kernel) and the one mmg_cnblock_plan names for this device, on the grid cnblock_ref.plan gives, no output holds a NaN fill, every sentinel tail is intact, rows that are equal (the rows have period P)
give equal bits, and the tile-loop cases give every workgroup (wave) at least two tiles at this device's CU count.

What these tests found: no wrong result.  On the parent's kernels every integer case was bit-exact and every gaussian figure inside
its derived bar; the only bars missed on the first MI355X run were those that hold nothing but K_ACC, then still at 1 (rstd 1.47 in
seven cases, db2raw 3.31 at 32 832 rows) - the measurement cnblock_ref.K_ACC = 16 was set from.  Two host-side changes came with the
tests (csrc/cnblock_bwdw.hip): MMG_BWDW_W12 is read per call, and the kernel note names both launches."""
import pytest
import torch

from tests import cnblock_ref as R
from tests.conftest import measured

pytestmark = pytest.mark.gpu
BF, F64, F32 = R.BF, R.F64, torch.float32
NAME = "cnblock_f64_"
OUT_FILL, TAIL_FILL = 0x7FC1, 0x5A5A                   # bf16 NaN bits in every output; sentinel bits of the rows past its end
OUT_FILL32, TAIL_FILL32 = 0x7FC00001, 0x5A5A5A5A       # the same for the fp32 row statistics
EXTRA = 128                                            # rows past the last one: a whole workgroup tile


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


def _out(M, cols, dev, fp32=False):
    """[M + EXTRA, cols] (fp32: [M + EXTRA]) output buffer: NaN bits in the rows the kernel owns, sentinel bits past them."""
    if fp32:
        buf = torch.full((M + EXTRA,), OUT_FILL32, dtype=torch.int32, device=dev)
        buf[M:] = TAIL_FILL32
        return buf.view(F32)
    buf = torch.full((M + EXTRA, cols), OUT_FILL, dtype=torch.int16, device=dev)
    buf[M:] = TAIL_FILL
    return buf.view(BF)


def _tail_ok(buf, M):
    if buf.dtype == F32:
        return bool((buf[M:].view(torch.int32) == TAIL_FILL32).all())
    return bool((buf[M:].view(torch.int16) == TAIL_FILL).all())


def _rows(t, src, dev):
    """Base rows [n, C] float64 -> the M periodic rows, bf16 on the device."""
    return t.to(F32).to(BF).to(dev)[src].contiguous()


def _f32(t, dev):
    return t.to(F32).contiguous().to(dev)


def _launch(case, d, M, dev):
    """The case's launch -> ({output: device buffer with its tail}, {accumulated output: device tensor}, kernel noted)."""
    from mmgclip import _hip, kernels as Kn
    call, ptr, stream = _hip.call, _hip.ptr, _hip.stream
    C, H4 = case.C, 4 * case.C
    n = d["xd"].shape[0]
    src = (torch.arange(M) % n).to(dev)
    xd = _rows(d["xd"], src, dev)
    lnw, lnb, b1 = _f32(d["ln_w"], dev), _f32(d["ln_b"], dev), _f32(d["b1"], dev)
    w1, w2, ls = _f32(d["w1"], dev), _f32(d["w2"], dev), _f32(d["ls"], dev)
    eps = float(d["eps"])
    outs, accs = {}, {}
    lib = _hip.load()
    if case.op == "fwd":
        packed = Kn.cnblock_pack(w1, w2)
        res, b2 = _rows(d["res"], src, dev), _f32(d["b2"], dev)
        outs["y"] = _out(M, C, dev)
        if case.save:
            outs.update(hpre=_out(M, H4, dev), mean=_out(M, 0, dev, True), rstd=_out(M, 0, dev, True))
        if case.save >= 2:
            outs["xln"] = _out(M, C, dev)
        if case.save >= 3:
            outs["gact"] = _out(M, H4, dev)
        g = lambda k: ptr(outs[k]) if k in outs else None
        fn = lambda: call("mmg_cnblock_mlp_fwd", ptr(xd), ptr(lnw), ptr(lnb), eps, ptr(packed), ptr(b1), ptr(b2), ptr(ls), ptr(res), g("y"),
                          g("hpre"), g("xln"), g("gact"), g("mean"), g("rstd"), 1 if case.save == 4 else 0, M, C, stream())
    elif case.op == "bwd":
        mode = Kn.cnblock_bwd_mode(C)
        packed = Kn.cnblock_pack(w1, w2, ls, backward=mode)
        dy = _rows(d["dy"], src, dev)
        hsaved = _rows(d["hsaved"], src, dev) if mode == 2 else None
        outs.update(dh=_out(M, H4, dev), g=_out(M, H4, dev), xln=_out(M, C, dev), dxln=_out(M, C, dev), mean=_out(M, 0, dev, True),
                    rstd=_out(M, 0, dev, True))
        if case.ln:
            accs = {k: torch.full((C,), R.FILL[k], dtype=F32, device=dev) for k in ("ln_dw", "ln_db")}
        fn = lambda: call("mmg_cnblock_mlp_bwd", ptr(dy), ptr(xd), ptr(lnw), ptr(lnb), eps, ptr(packed), ptr(b1), ptr(hsaved), ptr(outs["dh"]),
                          ptr(outs["g"]), ptr(outs["xln"]), ptr(outs["dxln"]), ptr(outs["mean"]), ptr(outs["rstd"]), ptr(accs.get("ln_dw")),
                          ptr(accs.get("ln_db")), M, C, stream())
    else:
        packed, b1f = Kn.cnblock_bwdw_pack(w1, w2, lnw, lnb, ls, b1)
        dy = _rows(d["dy"], src, dev)
        outs["dd"] = _out(M, C, dev)
        shapes = dict(dW1=(H4, C), db1=(H4,), dW2raw=(C, H4), db2raw=(C,), ln_dw=(C,), ln_db=(C,))
        accs = {k: torch.full(s, R.FILL[k], dtype=F32, device=dev) for k, s in shapes.items()}
        fn = lambda: call("mmg_cnblock_bwdw", ptr(dy), ptr(xd), ptr(lnw), ptr(lnb), eps, ptr(packed), ptr(b1f), ptr(outs["dd"]),
                          ptr(accs["dW1"]), ptr(accs["db1"]), ptr(accs["dW2raw"]), ptr(accs["db2raw"]), ptr(accs["ln_dw"]), ptr(accs["ln_db"]),
                          M, C, stream())
    _sync()
    lib.mmg_set_kernel_notes(1)
    try:
        fn()
        name = lib.mmg_last_kernel().decode()
    finally:
        lib.mmg_set_kernel_notes(0)
    _sync()
    if case.op == "bwdw":
        accs = dict(accs, b1f=b1f)
    return outs, accs, name


def _run(case, dev, monkeypatch, d=None):
    from mmgclip import _hip
    _set_env(monkeypatch, case.env)
    cus = _hip.load().mmg_device_cu_count()
    M = R.rows(case, cus)
    if d is None:
        d = R.prepared(case, cus)[0]
    return _launch(case, d, M, dev) + (M,)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_kernels_against_float64(case, dev, monkeypatch):
    """Every row of the table: bit-exact where cnblock_ref.exact_outputs says so, inside the derived bars elsewhere; the launch is the
    instantiation the table names; tails, fills and equal rows as the module docstring lists them."""
    from mmgclip import _hip
    cus = _hip.load().mmg_device_cu_count()
    pl = R.plan(case, cus)
    if case.loop:
        print(case.id, "tiles per walker", pl["min_tiles"], "-", pl["max_tiles"], "on", cus, "CUs;", pl["M"], "rows")
        assert pl["min_tiles"] >= 2 and pl["ntiles"] > 2 * pl["walkers"], (cus, pl)
    d, ref, bar = R.prepared(case, cus)
    if case.loop and case.regime == "integer":        # (the row count follows the CU count: the CPU file checked it at 256)
        assert R.exactness_violations(case, d, pl["M"]) == [], cus
    outs, accs, name, M = _run(case, dev, monkeypatch)
    n = d["xd"].shape[0]
    bad, vals = [], {}
    rows_out, acc_out = R.outputs_of(case)
    assert set(outs) | set(accs) == set(rows_out) | set(acc_out), (sorted(outs), sorted(accs))
    src = (torch.arange(M) % n).to(dev)
    for k, buf in outs.items():
        if not _tail_ok(buf, M):
            bad.append(f"{k}: rows past the end were written")
        body = buf[:M]
        if not bool(torch.isfinite(body).all()):
            bad.append(f"{k}: {int((~torch.isfinite(body)).sum())} elements unwritten (NaN fill) or not finite")
        bits = body.view(torch.int32 if body.dtype == F32 else torch.int16)
        if M > n and not torch.equal(bits, bits[:n][src]):
            bad.append(f"{k}: equal rows gave different bits")
        got = body[:n].cpu().to(F64)
        worst, differ = R.check(case, k, got, ref[k], bar[k])
        vals[k + "_ratio"], vals[k + "_differ"] = worst, differ
    for k, t in accs.items():
        worst, differ = R.check(case, k, t.cpu().to(F64), ref[k], bar[k])
        vals[k + "_ratio"], vals[k + "_differ"] = worst, differ
    print(case.id, vals, name)
    measured(NAME + case.id, kernel=name, rows=M, k_acc=R.K_ACC, **vals)
    exact = R.exact_outputs(case)
    for k in list(outs) + list(accs):
        if not vals[k + "_ratio"] <= 1.0:
            bad.append(f"{k}: " + ("not bit-exact" if k in exact else f"worst ratio {vals[k + '_ratio']} > 1")
                       + f" ({vals[k + '_differ']:.5f} of the elements differ from the reference cast to the output type)")
    if name != R.kernel_note(case):
        bad.append(f"launched {name!r}, the table says {R.kernel_note(case)!r}")
    planned = _hip.load().mmg_cnblock_plan(*R.plan_args(case, cus)[:5], 0).decode()          # (the knobs are still the case's; cus = 0: this device)
    if planned.split(" grid=")[0] != name or f" grid={pl['grid']} " not in planned:
        bad.append(f"launched {name!r} on a grid of {pl['grid']}, mmg_cnblock_plan says {planned!r}")
    assert not bad, bad


def _bits(outs, M):
    return {k: v[:M].view(torch.int32 if v.dtype == F32 else torch.int16).clone() for k, v in outs.items()}


@pytest.mark.parametrize("M", [417, 1, 32 * 25 + 7])
def test_three_forward_forms_at_96_give_the_same_bits(M, dev, monkeypatch):
    """Streaming, 8 and 12 resident waves: the per-row arithmetic order is the same (chunk, 32-unit group, k-step, tile; shown on the
    emulation by test_cnblock_ref_cpu), so y of gaussian data is identical."""
    base = R.Case("fwd", 96, M, "gaussian")
    first = None
    for res in (0, 8, 12):
        c = base._replace(res=res)
        outs, _, name, _ = _run(c, dev, monkeypatch)
        assert name == R.kernel_note(c) and _tail_ok(outs["y"], M) and bool(torch.isfinite(outs["y"][:M]).all()), (name, res)
        y = _bits(outs, M)["y"]
        first = y if first is None else first
        assert torch.equal(y, first), res


@pytest.mark.parametrize("op,C", [("fwd", 96), ("fwd", 192), ("fwd", 512), ("bwd", 96), ("bwd", 128), ("bwd", 384)])
def test_nontemporal_stores_give_the_same_bits(op, C, dev, monkeypatch):
    base = R.Case(op, C, 2 * R.BM + 16 * R.mt(C) + 3, "gaussian", save=4 if op == "fwd" else 0)
    runs = []
    for nt in (0, 1):
        outs, _, name, M = _run(base._replace(nt=nt), dev, monkeypatch)
        assert all(_tail_ok(v, M) for v in outs.values())
        runs.append(_bits(outs, M))
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0]), [k for k in runs[0] if not torch.equal(runs[0][k], runs[1][k])]


@pytest.mark.parametrize("C", R.BWD_WIDTHS)
def test_forward_and_backward_give_the_same_statistics_and_layernorm_output(C, dev, monkeypatch):
    """mmg_cnblock_mlp_fwd and mmg_cnblock_mlp_bwd run the same LayerNorm code on the same rows: mean, rstd and xln are identical."""
    b = R.Case("bwd", C, 2 * R.BM + 16 * R.mt(C) + 3, "gaussian")
    d = R.prepared(b)[0]
    ob, _, _, M = _run(b, dev, monkeypatch, d)
    of, _, _, _ = _run(b._replace(op="fwd", save=2), dev, monkeypatch, d)
    bb, bf = _bits(ob, M), _bits(of, M)
    assert all(torch.equal(bb[k], bf[k]) for k in ("mean", "rstd", "xln")), [k for k in ("mean", "rstd", "xln") if not torch.equal(bb[k], bf[k])]


@pytest.mark.parametrize("case", [R.Case("fwd", 96, 32 * 25 + 7, "gaussian"), R.Case("fwd", 128, 2 * R.BM + 35, "gaussian", save=4),
                                  R.Case("fwd", 384, 2 * R.BM + 19, "gaussian", save=3), R.Case("bwd", 192, 2 * R.BM + 35, "gaussian"),
                                  R.Case("bwd", 384, 2 * R.BM + 19, "gaussian"), R.Case("bwdw", 96, 64 * 5, "gaussian")], ids=lambda c: c.id)
def test_outputs_without_atomics_give_the_same_bits_run_to_run(case, dev, monkeypatch):
    """Nothing but the fp32 accumulators depends on when a workgroup runs: every other output, three times."""
    runs = []
    for _ in range(3):
        outs, _, _, M = _run(case, dev, monkeypatch)
        runs.append(_bits(outs, M))
    assert all(torch.equal(runs[0][k], r[k]) for r in runs[1:] for k in runs[0])
