"""tests/layernorm_ref.py without a GPU: the table reaches every instantiation of the kernel table (csrc/layernorm_plan.h) and every call mode, the kernel
notes are spelt as the launcher spells them, torch.equal is justified where the table uses it (on the reference alone), the fp8
boundary share is within its cap, the emulation of the kernels' arithmetic is inside every bar on every case (exact where the table says
exact), and each subtly wrong variant of it leaves the bars on every case that contains the feature it breaks.  (That the restated
selection agrees with the library's ln_plan is checked in tests/test_layernorm_plan_cpu.py, without a GPU; tests/test_layernorm_gpu.py
compares the kernel note of every launch with both.)"""
import pytest
import torch

from tests import layernorm_ref as R

UNIQUE = list({c._replace(strided="", pad=8): c._replace(strided="", pad=8) for c in R.CASES}.values())


def test_every_instantiation_is_launched_in_both_regimes():
    assert len(R.ALL_INSTANTIATIONS) == 28
    for regime in ("integer", "gaussian"):
        seen = {R.instantiation(c) for c in R.CASES if c.regime == regime}
        assert seen == R.ALL_INSTANTIATIONS, (R.ALL_INSTANTIATIONS - seen, seen - R.ALL_INSTANTIATIONS)
    assert len({c.id for c in R.CASES}) == len(R.CASES)
    # what the selection can produce at all: every width, mode and knob value
    for C in range(8, 4097, 8):
        for op in ("fwd", "bwd"):
            for plain in (None, 0):
                for ch3 in (None, 0):
                    for x32 in (False, True):
                        assert R.instantiation(R.Case(op, C, 64, "integer", x32=x32, plain=plain, ch3=ch3)) in R.ALL_INSTANTIATIONS


def test_kernel_notes_are_spelt_as_the_launcher_spells_them():
    note = lambda **kw: R.kernel_note(R.Case(**{"regime": "integer", "M": 64, **kw}))
    assert note(op="fwd", C=96) == "layernorm_fwd_plain_kernel<4>"
    assert note(op="fwd", C=96, plain=0) == "layernorm_fwd_kernel<16, 1>"
    assert note(op="fwd", C=768) == "layernorm_fwd_plain_kernel<32>"
    assert note(op="fwd", C=768, plain=0) == "layernorm_fwd_kernel<32, 3>"
    assert note(op="fwd", C=768, plain=0, ch3=0) == "layernorm_fwd_kernel<64, 2>"
    assert note(op="fwd", C=768, x32=True) == "layernorm_fwd_kernel<32, 3>"
    assert note(op="fwd", C=768, fp8=True, ch3=0) == "layernorm_fwd_kernel<64, 2>"
    assert note(op="fwd", C=1536, plain=0, ch3=0) == "layernorm_fwd_kernel<64, 4>"
    assert note(op="bwd", C=1536) == "layernorm_bwd_plain_kernel<64>"
    assert note(op="bwd", C=1536, add=True) == "layernorm_bwd_kernel<64, 4>"
    assert note(op="bwd", C=384, plain=0) == "layernorm_bwd_kernel<64, 1>"
    assert note(op="bwd", C=8) == "layernorm_bwd_kernel<8, 1>"
    assert note(op="bwd", C=72) == "layernorm_bwd_kernel<16, 1>"
    assert note(op="fwd", C=3072) == "layernorm_fwd_kernel<64, 8>" and note(op="fwd", C=4096) == "layernorm_fwd_kernel<64, 8>"
    assert note(op="fwd", C=1032) == "layernorm_fwd_kernel<64, 4>" and note(op="bwd", C=2056) == "layernorm_bwd_kernel<64, 8>"
    with pytest.raises(ValueError):
        note(op="fwd", C=4104)


def test_axes_of_the_table():
    """Widths, modes at a plain-eligible and a generic-only width, strides, row counts, the two launch-size paths, the flavours."""
    assert {c.C for c in R.CASES} == set(R.WIDTHS)
    for wide in (True, False):
        at = [c for c in R.CASES if (R.select(c._replace(x32=False, res=False, yf=False, fp8=False, add=False))[0] == "plain") == wide
              and c.plain is None]
        f = [c for c in at if c.op == "fwd"]
        b = [c for c in at if c.op == "bwd"]
        for regime in ("integer", "gaussian"):
            fr, br = [c for c in f if c.regime == regime], [c for c in b if c.regime == regime]
            assert {(c.x32, c.res, c.yf) for c in fr} >= {(False, False, False), (True, False, False), (True, True, False),
                                                         (True, False, True), (True, True, True)}, (wide, regime)
            assert any(c.fp8 for c in fr) and any(not c.stats for c in fr)
            assert {(c.patch[0] % 2, c.patch[1] % 2) for c in fr if c.patch} == {(0, 0), (1, 0), (0, 1), (1, 1)}
            assert {(c.add, c.grads) for c in br} == {(a, g) for a in (False, True) for g in (False, True)}
            assert {(c.add, c.grads) for c in br if c.x32} == {(a, g) for a in (False, True) for g in (False, True)}
            assert any(c.patch and c.add for c in br)
            assert {c.strided for c in fr} >= {"x", "y", "res", "yf"} and {c.strided for c in br} >= {"x", "dy", "dx", "add"}
            assert any(c.patch and c.strided == "y" for c in fr) and any(c.patch and c.strided == "dy" for c in br)
    assert {c.pad for c in R.CASES if c.strided} == {8, 64}
    for c in R.CASES:
        pl = R.plan(c)
        assert (c.M * c.C * 2 >= 2 ** 28) == pl["nt"] or c.x32 or c.fp8
        if c.patch:
            assert c.M % (c.patch[0] * c.patch[1]) == 0 and c.M <= R.P
    assert any(c.M == 1 and R.select(c)[1] == 4 for c in R.CASES)
    assert any(c.M % R.plan(c)["rpb"] == 0 and not c.patch for c in R.CASES)
    plainly = [c for c in R.CASES if not c.patch]
    ragged = [c for c in plainly if (c.M % R.plan(c)["rpw"] or R.plan(c)["rpw"] == 1) and c.M % R.plan(c)["rpb"]
              and R.plan(c)["blocks"] in (3, 4)]
    assert len(ragged) >= len(plainly) * 3 // 4, (len(ragged), len(plainly))      # (the rest: the cases above and below, and fp8)
    for op in ("fwd", "bwd"):
        for kind in ("plain", "generic"):
            for regime in ("integer", "gaussian"):
                sel = [c for c in R.CASES if c.op == op and R.select(c)[0] == kind and c.regime == regime]
                loop = [c for c in sel if R.plan(c)["capped"] and not R.plan(c)["nt"]]
                assert loop and all(R.plan(c)["iters"] == 2 and c.M > R.CAP[op] * R.plan(c)["rpb"] for c in loop), (op, kind)
                assert any(R.plan(c)["nt"] for c in sel), (op, kind)
    assert {c.eps for c in R.CASES if c.regime == "gaussian"} == {1e-6, 1e-12, 1e-5}
    assert all(c.eps == 1e-12 for c in R.CASES if c.regime == "gaussian" and c.x32)
    assert all(c.eps == 1e-5 for c in R.CASES if c.regime == "gaussian" and not c.x32 and c.C in (256, 512))
    d = R.make_data(R.Case("fwd", 96, 200, "gaussian"))
    x = d["xs"]
    assert float(x[1].mean()) > 90 and float(x[2].var()) == 0 and 0 < float(x[3].abs().max()) < 2.0 ** -17
    d = R.make_data(R.Case("fwd", 256, 200, "gaussian", x32=True, res=True, eps=1e-12))
    assert float(d["xs"][2].var()) == 0 and float(d["x"][2].var()) > 0 and not torch.equal(R._rb(d["x"]), d["x"])
    assert 0.1 < float(d["xs"][3].var()) / 1e-12 < 10


def test_patch_map_is_a_permutation_that_drops_the_odd_edge():
    for H, W in ((4, 6), (5, 6), (4, 7), (5, 7)):
        M = 3 * H * W
        rows = torch.arange(M * 8, dtype=R.F64).reshape(M, 8) + 1
        mat = R.to_patch(rows, H, W)
        assert mat.shape == (3 * (H // 2) * (W // 2), 32) and bool((mat != 0).all())
        back = R.from_patch(mat, M, H, W)
        live = R.patch_map(M, H, W)[0]
        assert int(live.sum()) == 3 * (H & ~1) * (W & ~1) and torch.equal(back[live], rows[live]) and bool((back[~live] == 0).all())
    # row (n, h, w) -> patch row (n, h/2, w/2), columns ((h&1) 2 + (w&1)) C ...
    live, prow, quad = R.patch_map(2 * 4 * 6, 4, 6)
    m = 1 * 24 + 3 * 6 + 4
    assert (int(prow[m]), int(quad[m])) == ((1 * 2 + 1) * 3 + 2, 2)


def test_e4m3_quantiser_agrees_with_torch():
    v = torch.cat([torch.randn(20000, generator=torch.Generator().manual_seed(1), dtype=R.F64) * s for s in (1e-3, 0.1, 1, 30, 300)])
    v = torch.cat([v, torch.tensor([0.0, 448.0, -448.0, 500.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 0.0009765625 * 1.5], dtype=R.F64)])
    mine = R.q8(R._r32(v))
    theirs = R._r32(v).clamp(-448, 448).to(torch.float32).to(torch.float8_e4m3fn).to(R.F64)
    assert torch.equal(mine, theirs)


@pytest.mark.parametrize("case", [c for c in UNIQUE if c.regime == "integer"], ids=lambda c: c.id)
def test_integer_regime_is_exact_by_construction(case):
    d, ref, bar, ebar = R.prepared(case)
    assert R.exactness_violations(case, d, ref, ebar) == []


@pytest.mark.parametrize("case", [c for c in UNIQUE if c.fp8], ids=lambda c: c.id)
def test_fp8_boundary_share_is_within_its_cap(case):
    d, ref, bar, ebar = R.prepared(case)
    share = R.fp8_boundary_share(ref["y"], ebar["y"])
    assert share <= 0.01, share
    if case.regime == "integer":
        assert share == 0.0


def _ratios(case, out, ref, bar):
    return {k: R.check(case, k, out[k], ref[k], bar[k])[0] for k in R.outputs_of(case)}


@pytest.mark.parametrize("case", UNIQUE, ids=lambda c: c.id)
def test_emulation_is_inside_every_bar_and_every_mutation_leaves_them(case):
    d, ref, bar, _ = R.prepared(case)
    out = R.emulate(case, d)
    assert set(out) == set(R.outputs_of(case))
    res = _ratios(case, out, ref, bar)
    assert all(v <= 1.0 for v in res.values()), res
    assert all(res[k] == 0.0 for k in R.exact_outputs(case) if k in res), res
    if case.yf:
        assert torch.equal(out["y"], R._rb(out["yf"]))
    missed = []
    for mut in R.MUTATIONS:
        if R.mutation_applies(case, mut):
            res = _ratios(case, R.emulate(case, d, mut), ref, bar)
            if not any(not v <= 1.0 for v in res.values()):
                missed.append((mut, max(res.values())))
    assert not missed, missed


def test_every_mutation_is_exercised():
    for mut in R.MUTATIONS:
        for regime in ("integer", "gaussian"):
            hit = [c for c in UNIQUE if c.regime == regime and R.mutation_applies(c, mut)]
            assert hit or (regime, mut) in (("integer", "yf_after_bf16"), ("integer", "neighbour_stats")), (mut, regime)


def test_fp32_row_kernel_on_bf16_exact_rows_is_the_bf16_row_kernel():
    """What the same-bits GPU test rests on: with bf16-exact rows the two entry points differ in the load alone, so where they run the
    same instantiation the emulation gives the same y."""
    a = R.Case("fwd", 256, 37, "gaussian")
    b = a._replace(x32=True)
    assert R.instantiation(a) == R.instantiation(b)
    d = R.make_data(a)
    assert torch.equal(R.emulate(a, d)["y"], R.emulate(b, d)["y"])
