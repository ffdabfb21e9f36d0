"""tests/cnblock_ref.py without a GPU: the table launches every template instantiation of the fused CNBlock MLP kernels in the integer
regime, torch.equal is justified where the table uses it (on the reference alone), the emulation of the kernels' arithmetic is inside
every bar on every case (exact where the table says exact), and each subtly wrong variant of it leaves the bars on every case that
contains the feature it breaks.  The tile-loop cases run here on a 2-CU device (same launch rules, fewer rows)."""
import pytest
import torch

from tests import cnblock_ref as R

CUS = 2


def _shape_key(c):
    return (c.op, c.C, c.M, c.regime, 4 if c.save == 4 else 3 if c.save else 0, c.ln, R.resident(c))


UNIQUE = list({_shape_key(c): c for c in R.CASES}.values())


def test_every_instantiation_is_launched_in_the_integer_regime():
    seen = {i for c in R.CASES if c.regime == "integer" for i in R.instantiations(c)}
    assert len(R.ALL_INSTANTIATIONS) == 14 + 8 + 6
    assert seen == R.ALL_INSTANTIATIONS, (R.ALL_INSTANTIATIONS - seen, seen - R.ALL_INSTANTIATIONS)
    assert len({c.id for c in R.CASES}) == len(R.CASES)


def _library_note(monkeypatch, **kw):
    """The same spelling from the library's own plan (mmg_cnblock_plan: no launch, no GPU), under the case's knobs."""
    from mmgclip import _hip
    case = R.Case(**{"regime": "integer", "M": 64, **kw})
    for name, v in case.env.items():
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    return _hip.load().mmg_cnblock_plan(*R.plan_args(case, 256)).decode().split(" grid=")[0]


def test_kernel_notes_are_spelt_as_the_launchers_spell_them(monkeypatch):
    note = lambda **kw: R.kernel_note(R.Case(**{"regime": "integer", "M": 64, **kw}))
    _check_the_eight_spellings(note)
    _check_the_eight_spellings(lambda **kw: _library_note(monkeypatch, **kw))


def _check_the_eight_spellings(note):
    assert note(op="fwd", C=96) == "cnblock_mlp_fwd_kernel<96, false, 12>"
    assert note(op="fwd", C=96, res=8) == "cnblock_mlp_fwd_kernel<96, false, 8>"
    assert note(op="fwd", C=96, res=0) == "cnblock_mlp_fwd_kernel<96, false>"
    assert note(op="fwd", C=96, save=2) == "cnblock_mlp_fwd_kernel<96, true>"
    assert note(op="bwd", C=384, ln=True) == "cnblock_mlp_bwd_kernel<384, false, true>"
    assert note(op="bwd", C=128) == "cnblock_mlp_bwd_kernel<128, true, false>"
    assert note(op="bwdw", C=96) == "cnblock_bwdw_kernel<96, 1, 8, 2> + <96, 2, 8, 1>"
    assert note(op="bwdw", C=96, w12=1, var=2, hto=0) == "cnblock_bwdw_kernel<96, 1, 12, 0> + <96, 2, 8, 0>"


def test_axes_of_the_table():
    """Every tail edge per width and entry point, the knobs, the row flavours, and tile loops that give every walker two tiles."""
    for op, widths in (("fwd", R.WIDTHS), ("bwd", R.BWD_WIDTHS)):
        for C in widths:
            Ms = {c.M for c in R.CASES if c.op == op and c.C == C and c.regime == "integer" and not R.resident(c)}
            assert {1, 17, 16 * R.mt(C) + 1, R.BM - 1, R.BM + 1, 2 * R.BM + 16 * R.mt(C) + 3, 0} <= Ms, (op, C, Ms)
            assert any(c.regime == "gaussian" and c.loop is False for c in R.CASES if c.op == op and c.C == C)
    assert {c.save for c in R.CASES if c.op == "fwd"} == {0, 1, 2, 3, 4}
    assert {(c.var, c.hto) for c in R.CASES if c.op == "bwdw"} >= {(v, h) for v in (0, 1, 2) for h in (0, 1)}
    for op in ("fwd", "bwd", "bwdw"):
        assert any(c.loop and c.regime == "gaussian" for c in R.CASES if c.op == op)
        assert {c.nt for c in R.CASES if c.op == op and op != "bwdw"} in ({None, 0, 1}, set())
    for cus in (CUS, 256, 304):
        for c in R.CASES:
            pl = R.plan(c, cus)
            if c.loop:
                assert pl["min_tiles"] >= 2 and pl["ntiles"] > 2 * pl["walkers"], (c.id, cus, pl)
            rw = R.resident(c)
            if rw and c.M == 32 * rw + 33:                     # the last workgroup has waves without a tile
                assert pl["grid"] == 2 and pl["ntiles"] == rw + 2
    for rw in (8, 12):
        assert any(R.resident(c) == rw and c.loop for c in R.CASES)
    d = R.make_data(R.Case("fwd", 96, 200, "gaussian"))
    x = d["xd"]
    assert float(x[1].mean()) > 90 and float(x[2].var()) == 0 and 0 < float(x[3].abs().max()) < 2.0 ** -17


@pytest.mark.parametrize("case", [c for c in UNIQUE if c.regime == "integer"], ids=lambda c: c.id)
def test_integer_regime_is_exact_by_construction(case):
    d, _, _ = R.prepared(case, 256)
    assert R.exactness_violations(case, d, R.rows(case, 256)) == []


def _ratios(case, out, ref, bar):
    M = next(v.shape[0] for k, v in out.items() if k in ("y", "dd", "xln"))
    ref, bar = R.expand(case, ref, bar, M)
    rows_out, accs = R.outputs_of(case)
    return {k: R.check(case, k, out[k], ref[k], bar[k])[0] for k in rows_out + accs}


@pytest.mark.parametrize("case", UNIQUE, ids=lambda c: c.id)
def test_emulation_is_inside_every_bar_and_every_mutation_leaves_them(case):
    d, ref, bar = R.prepared(case, CUS)
    res = _ratios(case, R.emulate(case, d, CUS), ref, bar)
    assert all(v <= 1.0 for v in res.values()), res
    if case.regime == "integer":
        assert all(res[k] == 0.0 for k in R.exact_outputs(case) if k in res), res
    missed = []
    for mut in R.MUTATIONS:
        if R.mutation_applies(case, mut, CUS):
            res = _ratios(case, R.emulate(case, d, CUS, mut), ref, bar)
            if not any(not v <= 1.0 for v in res.values()):
                missed.append((mut, max(res.values())))
    assert not missed, missed


def test_every_mutation_is_exercised():
    for mut in R.MUTATIONS:
        for op in ("fwd", "bwd", "bwdw"):
            hit = [c for c in UNIQUE if c.op == op and R.mutation_applies(c, mut, CUS)]
            assert hit or mut in {"fwd": ("tail_rows_counted", "b1f_twice", "dW1_no_db1_term", "ls_missing_dG", "gelu_grad_sign"),
                                  "bwd": ("no_colperm", "b2_dropped", "ls_dropped", "res_dropped", "b1f_twice", "dW1_no_db1_term"),
                                  "bwdw": ("pack_swap4", "no_colperm", "b1_packed", "b2_dropped", "ls_dropped", "res_dropped", "stale_chunk",
                                           "clamp_leak", "tail_rows_counted", "last_block_unwritten")}[op], (mut, op)


def test_resident_and_streaming_forward_share_the_per_row_arithmetic_order():
    """What the same-bits GPU test rests on: at C = 96 the three forward forms differ in which wave owns a row and in where the weight
    images live, not in the per-row sequence - chunk, 32-unit group, k-step, tile - so the emulation of a row does not depend on them."""
    base = R.Case("fwd", 96, 417, "gaussian")
    d, _, _ = R.prepared(base)
    outs = [R.emulate(base._replace(res=r), d, CUS)["y"] for r in (0, 8, 12)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
