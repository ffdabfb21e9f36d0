"""The LayerNorm host layer's plans (csrc/layernorm_plan.hip), read through mmg_layernorm_plan: no GPU, nothing is launched.

What a plan string holds: the kernel instantiation as mmg_last_kernel() spells it, then " grid=N block=256 lds=B nt=0|1".  The plans are
compared with three things that do not come from the code under test: the Python restatement of the rules (layernorm_ref.select / plan),
the kernels the launcher BEFORE this host layer launched on an MI355X for every case of layernorm_ref.CASES
(profiles/layernorm_measured_tolerances.jsonl), and a literal table at the towers' own shapes."""
import json
import os

import pytest

from mmgclip import _hip
from tests import layernorm_ref as R

RECORDS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "layernorm_measured_tolerances.jsonl")

# (door, M, C, res, yf, add) -> plan under default knobs; door 0 mmg_layernorm_fwd, 1 _fwd_f32, 2 _fwd_fp8, 3 _bwd, 4 _bwd_f32.  ConvNeXt-T
# (96 ... 768) and ConvNeXt-B (128 ... 1024) at the pixel rows of 64 images of 224 x 224 per stage; BERT's fp32-row LayerNorms at 128 x 77
# tokens; ViT-B/16 at 64 x 197 tokens (ln_1's backward takes `add`); a projection head (128 rows); C = 1024 at and one row below the
# 256 MiB of the streaming stores, which the fp32-row and fp8 entry points never take (C = 768 at 174 763 rows: above it).
SELECTION = {
    (0, 200704, 96, 0, 0, 0): 'layernorm_fwd_plain_kernel<4> grid=3136 block=256 lds=0 nt=0',
    (3, 200704, 96, 0, 0, 0): 'layernorm_bwd_plain_kernel<4> grid=1024 block=256 lds=768 nt=0',
    (0, 50176, 192, 0, 0, 0): 'layernorm_fwd_plain_kernel<8> grid=1568 block=256 lds=0 nt=0',
    (3, 50176, 192, 0, 0, 0): 'layernorm_bwd_plain_kernel<8> grid=1024 block=256 lds=1536 nt=0',
    (0, 12544, 384, 0, 0, 0): 'layernorm_fwd_plain_kernel<16> grid=784 block=256 lds=0 nt=0',
    (3, 12544, 384, 0, 0, 0): 'layernorm_bwd_plain_kernel<16> grid=784 block=256 lds=3072 nt=0',
    (0, 3136, 768, 0, 0, 0): 'layernorm_fwd_plain_kernel<32> grid=392 block=256 lds=0 nt=0',
    (3, 3136, 768, 0, 0, 0): 'layernorm_bwd_plain_kernel<32> grid=392 block=256 lds=6144 nt=0',
    (0, 200704, 128, 0, 0, 0): 'layernorm_fwd_kernel<16, 1> grid=4096 block=256 lds=0 nt=0',
    (3, 200704, 128, 0, 0, 0): 'layernorm_bwd_kernel<16, 1> grid=1024 block=256 lds=1024 nt=0',
    (0, 50176, 256, 0, 0, 0): 'layernorm_fwd_kernel<32, 1> grid=4096 block=256 lds=0 nt=0',
    (3, 50176, 256, 0, 0, 0): 'layernorm_bwd_kernel<32, 1> grid=1024 block=256 lds=2048 nt=0',
    (0, 12544, 512, 0, 0, 0): 'layernorm_fwd_kernel<64, 1> grid=3136 block=256 lds=0 nt=0',
    (3, 12544, 512, 0, 0, 0): 'layernorm_bwd_kernel<64, 1> grid=1024 block=256 lds=4096 nt=0',
    (0, 3136, 1024, 0, 0, 0): 'layernorm_fwd_kernel<64, 2> grid=784 block=256 lds=0 nt=0',
    (3, 3136, 1024, 0, 0, 0): 'layernorm_bwd_kernel<64, 2> grid=784 block=256 lds=8192 nt=0',
    (1, 9856, 768, 1, 1, 0): 'layernorm_fwd_kernel<32, 3> grid=1232 block=256 lds=0 nt=0',
    (4, 9856, 768, 0, 0, 1): 'layernorm_bwd_kernel<64, 2> grid=1024 block=256 lds=6144 nt=0',
    (0, 12608, 768, 0, 0, 0): 'layernorm_fwd_plain_kernel<32> grid=1576 block=256 lds=0 nt=0',
    (3, 12608, 768, 0, 0, 0): 'layernorm_bwd_plain_kernel<32> grid=1024 block=256 lds=6144 nt=0',
    (3, 12608, 768, 0, 0, 1): 'layernorm_bwd_kernel<64, 2> grid=1024 block=256 lds=6144 nt=0',
    (0, 128, 512, 0, 0, 0): 'layernorm_fwd_kernel<64, 1> grid=32 block=256 lds=0 nt=0',
    (3, 128, 512, 0, 0, 0): 'layernorm_bwd_kernel<64, 1> grid=32 block=256 lds=4096 nt=0',
    (0, 131072, 1024, 0, 0, 0): 'layernorm_fwd_kernel<64, 2> grid=4096 block=256 lds=0 nt=1',
    (0, 131071, 1024, 0, 0, 0): 'layernorm_fwd_kernel<64, 2> grid=4096 block=256 lds=0 nt=0',
    (3, 131072, 1024, 0, 0, 0): 'layernorm_bwd_kernel<64, 2> grid=1024 block=256 lds=8192 nt=1',
    (3, 131071, 1024, 0, 0, 0): 'layernorm_bwd_kernel<64, 2> grid=1024 block=256 lds=8192 nt=0',
    (1, 174763, 768, 0, 0, 0): 'layernorm_fwd_kernel<32, 3> grid=4096 block=256 lds=0 nt=0',
    (2, 174763, 768, 0, 0, 0): 'layernorm_fwd_kernel<32, 3> grid=4096 block=256 lds=0 nt=0',
}


def _set_env(monkeypatch, env):
    for name, v in env.items():
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _plan(door, M, C, res=0, yf=0, add=0):
    return _hip.load().mmg_layernorm_plan(door, M, C, res, yf, add).decode()


def _restated(case):
    """The plan string from layernorm_ref alone."""
    pl = R.plan(case)
    return f"{R.kernel_note(case)} grid={pl['blocks']} block=256 lds={2 * case.C * 4 if case.op == 'bwd' else 0} nt={int(pl['nt'])}"


def _case_of(args, plain=None, ch3=None):
    door, M, C, res, yf, add = args
    return R.Case("bwd" if door >= 3 else "fwd", C, M, "integer", x32=door in (1, 4), fp8=door == 2, res=bool(res), yf=bool(yf), add=bool(add),
                  plain=plain, ch3=ch3)


def _recorded():
    """test id -> kernel, as the launcher before the plan existed noted it on the device."""
    with open(RECORDS) as f:
        return {r["test"]: r["kernel"] for r in map(json.loads, f) if r["test"].startswith("layernorm_f64_")}


RECORDED = _recorded()


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_plan_is_the_restated_one_and_the_kernel_the_recorded_launch(case, monkeypatch):
    _set_env(monkeypatch, case.env)
    text = _plan(*case.plan_args)
    assert text == _restated(case)
    assert text.split(" grid=")[0] == RECORDED["layernorm_f64_" + case.id]


def test_every_case_has_a_recorded_launch():
    assert len(R.CASES) == 464
    assert not [c.id for c in R.CASES if "layernorm_f64_" + c.id not in RECORDED]


def test_the_table_names_exactly_the_built_kernels(monkeypatch):
    """Over the table, and over every width, entry point, mode and knob value: the 28 instantiations, no other."""
    note = {(op, kind, G, CH): (f"layernorm_{op}_plain_kernel<{G}>" if kind == "plain" else f"layernorm_{op}_kernel<{G}, {CH}>")
            for op, kind, G, CH in R.ALL_INSTANTIATIONS}
    assert len(set(note.values())) == 28
    seen = set()
    for case in R.CASES:
        _set_env(monkeypatch, case.env)
        seen.add(_plan(*case.plan_args).split(" grid=")[0])
    assert seen == set(note.values())
    for plain in (None, 0):
        for ch3 in (None, 0):
            _set_env(monkeypatch, {"MMG_LN_PLAIN": plain, "MMG_LN_CH3": ch3})
            for C in range(8, 4097, 8):
                for args in ((0, 64, C, 0, 0, 0), (1, 64, C, 0, 0, 0), (1, 64, C, 1, 1, 0), (2, 64, C, 0, 0, 0), (3, 64, C, 0, 0, 0),
                             (3, 64, C, 0, 0, 1), (4, 64, C, 0, 0, 0), (4, 64, C, 0, 0, 1)):
                    assert _plan(*args) == _restated(_case_of(args, plain, ch3)), (args, plain, ch3)


def test_selection_table(monkeypatch):
    """The literals were written out from layernorm_ref's restatement, which the launcher before this host layer matched on the device in
    every case of the table; each one is also held against that restatement and against the recorded launch of a table case with the same
    entry point, width, modes and knobs (the row count does not enter the choice of kernel)."""
    _set_env(monkeypatch, {"MMG_LN_PLAIN": None, "MMG_LN_CH3": None})
    wrong = {s: (_plan(*s), want) for s, want in SELECTION.items() if _plan(*s) != want}
    assert not wrong, wrong
    key = lambda c: (c.entry, c.C, c.res, c.yf, c.add, c.plain, c.ch3)
    launched = {}
    for c in R.CASES:
        launched.setdefault(key(c), set()).add(RECORDED["layernorm_f64_" + c.id])
    for s, want in SELECTION.items():
        case = _case_of(s)
        assert want == _restated(case), s
        assert launched[key(case)] == {want.split(" grid=")[0]}, s
    assert {(s[0], s[2]) for s in SELECTION} >= {(d, C) for d in (0, 3) for C in (96, 192, 384, 768, 128, 256, 512, 1024)}
    assert sorted(want[-4:] for s, want in SELECTION.items() if s[2] == 1024 and s[1] >= 131071 and s[0] in (0, 3)) == ["nt=0", "nt=0", "nt=1", "nt=1"]


KNOBS = [
    ({"MMG_LN_PLAIN": None, "MMG_LN_CH3": None}, "layernorm_fwd_plain_kernel<32>"),
    ({"MMG_LN_PLAIN": 1, "MMG_LN_CH3": 1}, "layernorm_fwd_plain_kernel<32>"),
    ({"MMG_LN_PLAIN": 0, "MMG_LN_CH3": None}, "layernorm_fwd_kernel<32, 3>"),
    ({"MMG_LN_PLAIN": None, "MMG_LN_CH3": 0}, "layernorm_fwd_plain_kernel<32>"),
    ({"MMG_LN_PLAIN": 0, "MMG_LN_CH3": 0}, "layernorm_fwd_kernel<64, 2>"),
    ({"MMG_LN_PLAIN": 0, "MMG_LN_CH3": 1}, "layernorm_fwd_kernel<32, 3>"),
]


def test_knobs(monkeypatch):
    """C = 768, forward: plain <32>; MMG_LN_PLAIN=0: the generic three-chunk rows; both 0: <64, 2>.  MMG_LN_CH3=0 alone changes the
    fp32-row entry point (never plain).  Unset equals 1, and the variables are read on every call."""
    for env, want in KNOBS:
        _set_env(monkeypatch, env)
        assert _plan(0, 3136, 768).split(" grid=")[0] == want, env
    _set_env(monkeypatch, {"MMG_LN_PLAIN": None, "MMG_LN_CH3": 0})
    assert _plan(1, 3136, 768).startswith("layernorm_fwd_kernel<64, 2> ")
    assert _plan(3, 3136, 768).startswith("layernorm_bwd_plain_kernel<32> ")
    _set_env(monkeypatch, {"MMG_LN_PLAIN": 0, "MMG_LN_CH3": None})
    assert _plan(1, 3136, 768).startswith("layernorm_fwd_kernel<32, 3> ")
    assert _plan(3, 3136, 768).startswith("layernorm_bwd_kernel<64, 2> ")
    assert len({want for _, want in KNOBS}) == 3


@pytest.mark.parametrize("door", range(5))
@pytest.mark.parametrize("M,C", [(16, 12), (16, 4104), (0, 256)])
def test_rejected_shapes_give_no_plan_and_the_entry_points_error(door, M, C):
    lib = _hip.load()
    assert _plan(door, M, C) == ""
    message = lib.mmg_last_error().decode()
    assert message.startswith(R.DOORS[door] + ":"), message
    assert "launch failed" not in message


@pytest.mark.parametrize("args", [(5, 16, 256, 0, 0, 0), (-1, 16, 256, 0, 0, 0), (0, 16, 256, 1, 0, 0), (2, 16, 256, 0, 1, 0), (1, 16, 256, 0, 0, 1)])
def test_unknown_door_or_mode_gives_no_plan(args):
    lib = _hip.load()
    assert _plan(*args) == "" and lib.mmg_last_error().decode().startswith("mmg_layernorm_plan:")
