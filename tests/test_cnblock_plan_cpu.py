"""The fused-CNBlock host layer's plans (csrc/cnblock_plan.hip), read through mmg_cnblock_plan with the CU count given: no GPU, nothing
is launched.

What a plan string holds: the kernel instantiation(s) as mmg_last_kernel() spells them, then " grid=G block=T lds=B nt=0|1 tiles=N"
(cnblock_bwdw: "block=(T1,T2)").  The plans are compared with three things that do not come from the code under test: the Python
restatement of the launchers' rules (cnblock_ref.plan_text), the kernels the launchers BEFORE this host layer noted on an MI355X for
every case of cnblock_ref.CASES (profiles/cnblock_measured_tolerances.jsonl), and a literal table at the towers' own shapes."""
import json
import os

import pytest

from mmgclip import _hip, kernels as K
from tests import cnblock_ref as R

RECORDS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cnblock_measured_tolerances.jsonl")
KNOBS = ("MMG_MLP_FWD_RES", "MMG_MLP_NT_STORE", "MMG_BWDW_VAR", "MMG_BWDW_HTO", "MMG_BWDW_W12")
DEFAULT = dict.fromkeys(KNOBS)
FWD, BWD, BWDW = 0, 1, 2

# (op, M, C, save, ln) -> plan on 256 CUs under default knobs.  64 images of 224 x 224: the pixel rows per stage of ConvNeXt-T (96, 192,
# 384) and ConvNeXt-B (128, 256, 512); each line worked out by hand from the launchers before this host layer:
#   tiles = ceil(M / 128) (resident forward at 96: ceil(M / 32); bwdw: M / 64)
#   grid  = min(tiles, per-CU workgroups x 256): forward 3 (96) / 2 (128, 192) / 1; backward 2 up to 192, else 1; resident forward
#           min(ceil(tiles / 12), 256); bwdw min(tiles, 256)
#   block = 256 up to C = 256, 512 beyond (8 waves of 16 rows); resident 64 x 12
#   lds   = 2 chunks x parts x (NC x C x 2 bytes) + 8 C floats, NC = 64 up to C = 128, else 32; parts = 2 (forward, backward at 384) or 3;
#           resident: all 4C / NC = 6 chunks
SELECTION = {
    (FWD, 200704, 96, 0, 0): "cnblock_mlp_fwd_kernel<96, false, 12> grid=256 block=768 lds=150528 nt=0 tiles=6272",
    (FWD, 200704, 96, 1, 0): "cnblock_mlp_fwd_kernel<96, true> grid=768 block=256 lds=52224 nt=0 tiles=1568",
    (FWD, 50176, 192, 0, 0): "cnblock_mlp_fwd_kernel<192, false> grid=392 block=256 lds=55296 nt=0 tiles=392",
    (FWD, 50176, 192, 1, 0): "cnblock_mlp_fwd_kernel<192, true> grid=392 block=256 lds=55296 nt=0 tiles=392",
    (FWD, 12544, 384, 0, 0): "cnblock_mlp_fwd_kernel<384, false> grid=98 block=512 lds=110592 nt=0 tiles=98",
    (FWD, 12544, 384, 1, 0): "cnblock_mlp_fwd_kernel<384, true> grid=98 block=512 lds=110592 nt=0 tiles=98",
    (BWD, 200704, 96, 0, 1): "cnblock_mlp_bwd_kernel<96, true, true> grid=512 block=256 lds=76800 nt=0 tiles=1568",
    (BWD, 50176, 192, 0, 0): "cnblock_mlp_bwd_kernel<192, true, false> grid=392 block=256 lds=79872 nt=0 tiles=392",
    (BWD, 12544, 384, 0, 0): "cnblock_mlp_bwd_kernel<384, false, false> grid=98 block=512 lds=110592 nt=0 tiles=98",
    (BWDW, 200704, 96, 0, 0): "cnblock_bwdw_kernel<96, 1, 8, 2> + <96, 2, 8, 1> grid=256 block=(512,512) lds=156032 nt=0 tiles=3136",
    (FWD, 200704, 128, 0, 0): "cnblock_mlp_fwd_kernel<128, false> grid=512 block=256 lds=69632 nt=0 tiles=1568",
    (FWD, 200704, 128, 1, 0): "cnblock_mlp_fwd_kernel<128, true> grid=512 block=256 lds=69632 nt=0 tiles=1568",
    (FWD, 50176, 256, 0, 0): "cnblock_mlp_fwd_kernel<256, false> grid=256 block=256 lds=73728 nt=0 tiles=392",
    (FWD, 50176, 256, 1, 0): "cnblock_mlp_fwd_kernel<256, true> grid=256 block=256 lds=73728 nt=0 tiles=392",
    (FWD, 12544, 512, 0, 0): "cnblock_mlp_fwd_kernel<512, false> grid=98 block=512 lds=147456 nt=0 tiles=98",
    (BWD, 200704, 128, 0, 1): "cnblock_mlp_bwd_kernel<128, true, true> grid=512 block=256 lds=102400 nt=0 tiles=1568",
    (BWD, 200704, 128, 0, 0): "cnblock_mlp_bwd_kernel<128, true, false> grid=512 block=256 lds=102400 nt=0 tiles=1568",
}
# the streaming stores' threshold: M x 4C x 2 bytes >= 256 MiB; at C = 192 that is M >= 174 762.67, at C = 384 M >= 87 381.33
NT_EDGE = [(BWD, 174763, 192, 0, 0, 1), (BWD, 174762, 192, 0, 0, 0), (BWD, 1 << 24, 96, 0, 0, 0), (BWD, 3000000, 96, 0, 1, 0),
           (FWD, 174763, 192, 1, 0, 0), (BWD, 87382, 384, 0, 0, 1), (BWD, 87381, 384, 0, 0, 0), (FWD, 174763, 192, 0, 0, 0)]


def _set_env(monkeypatch, env):
    for name, v in env.items():
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _plan(op, M, C, save=0, ln=0, cus=256):
    return _hip.load().mmg_cnblock_plan(op, M, C, save, ln, cus).decode()


def _kernel(text):
    return text.split(" grid=")[0]


def _recorded():
    """test id -> the kernels noted on the device by the launchers before the plan existed (a case was recorded more than once)."""
    out = {}
    with open(RECORDS) as f:
        for r in map(json.loads, f):
            if r["test"].startswith("cnblock_f64_"):
                out.setdefault(r["test"], set()).add(r["kernel"])
    return out


RECORDED = _recorded()
BY_ID = {"cnblock_f64_" + c.id: c for c in R.CASES}


@pytest.mark.parametrize("cus", [2, 256, 304])
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_plan_is_the_restated_one(case, cus, monkeypatch):
    _set_env(monkeypatch, case.env)
    assert _plan(*R.plan_args(case, cus)) == R.plan_text(case, cus)


@pytest.mark.parametrize("test", sorted(RECORDED))
def test_plan_names_the_kernel_of_the_recorded_launch(test, monkeypatch):
    assert test in BY_ID, f"{test}: a recorded launch without a case in cnblock_ref.CASES"
    case = BY_ID[test]
    _set_env(monkeypatch, case.env)
    assert {_kernel(_plan(*R.plan_args(case, 256)))} == RECORDED[test]


def test_every_case_has_a_recorded_launch():
    assert len(R.CASES) == 170 and len(RECORDED) == 170
    assert not [t for t in BY_ID if t not in RECORDED]


def test_the_table_names_exactly_the_built_kernels(monkeypatch):
    """Over the cases: the 28 instantiations of cnblock_ref.ALL_INSTANTIATIONS, no other."""
    spell = lambda i: f"{i[0]}<{R._spell(i[1:])}>"
    want = {spell(i) for i in R.ALL_INSTANTIATIONS}
    assert len(want) == 28
    seen = set()
    for case in R.CASES:
        _set_env(monkeypatch, case.env)
        first, _, second = _kernel(_plan(*R.plan_args(case, 256))).partition(" + ")
        seen.add(first)
        if second:
            seen.add("cnblock_bwdw_kernel" + second)
    assert seen == want


def test_selection_table(monkeypatch):
    """The literals against the library, against the restatement, and against the recorded launches of the table cases with the same
    entry point, width, modes and (default) knobs: the row count does not enter the choice of kernel."""
    _set_env(monkeypatch, DEFAULT)
    wrong = {s: (_plan(*s), want) for s, want in SELECTION.items() if _plan(*s) != want}
    assert not wrong, wrong
    op_name = ("fwd", "bwd", "bwdw")
    key = lambda c: (c.op, c.C, bool(c.save), c.ln)
    launched = {}
    for c in R.CASES:
        if all(v is None for v in c.env.values()):
            launched.setdefault(key(c), set()).update(RECORDED["cnblock_f64_" + c.id])
    for (op, M, C, save, ln), want in SELECTION.items():
        case = R.Case(op_name[op], C, M, "integer", save=save, ln=bool(ln))
        assert want == R.plan_text(case, 256), (op, M, C)
        if key(case) in launched:
            assert launched[key(case)] == {_kernel(want)}, (op, M, C)
    assert {(s[0], s[2]) for s in SELECTION} >= {(FWD, C) for C in R.WIDTHS} | {(BWD, C) for C in R.BWD_WIDTHS} | {(BWDW, 96)}


def test_streaming_stores(monkeypatch):
    """By rule: the backward from C = 128 up at 256 MiB of 4C-wide output, on both sides of the threshold; never at 96, never the
    forward.  MMG_MLP_NT_STORE=1 / 0 forces it on / off wherever something 4C-wide is stored: not in a forward that saves nothing."""
    nt = lambda text: int(text.split(" nt=")[1][0])
    _set_env(monkeypatch, DEFAULT)
    for op, M, C, save, ln, want in NT_EDGE:
        assert nt(_plan(op, M, C, save, ln)) == want, (op, M, C, save)
    stores_4c = [e for e in NT_EDGE if e[0] == BWD or e[3]]
    monkeypatch.setenv("MMG_MLP_NT_STORE", "1")
    assert [nt(_plan(*e[:5])) for e in stores_4c] == [1] * len(stores_4c)
    assert nt(_plan(FWD, 174763, 192, 0, 0)) == 0
    monkeypatch.setenv("MMG_MLP_NT_STORE", "0")
    assert [nt(_plan(*e[:5])) for e in NT_EDGE] == [0] * len(NT_EDGE)
    monkeypatch.setenv("MMG_MLP_NT_STORE", "7")           # any non-zero value: on
    assert nt(_plan(BWD, 64, 96)) == 1


@pytest.mark.parametrize("res,tail", [(None, "<96, false, 12> grid=256 block=768 lds=150528 nt=0 tiles=6272"),
                                      (12, "<96, false, 12> grid=256 block=768 lds=150528 nt=0 tiles=6272"),
                                      (8, "<96, false, 8> grid=256 block=512 lds=150528 nt=0 tiles=6272"),
                                      (0, "<96, false> grid=768 block=256 lds=52224 nt=0 tiles=1568"),
                                      (7, "<96, false> grid=768 block=256 lds=52224 nt=0 tiles=1568")])
def test_forward_resident_knob(res, tail, monkeypatch):
    """MMG_MLP_FWD_RES: 8 / 12 waves per workgroup of the resident forward, anything else the streaming form; C = 96 with nothing saved
    only."""
    _set_env(monkeypatch, dict(DEFAULT, MMG_MLP_FWD_RES=res))
    assert _plan(FWD, 200704, 96) == "cnblock_mlp_fwd_kernel" + tail
    assert _plan(FWD, 200704, 96, 1) == SELECTION[(FWD, 200704, 96, 1, 0)]
    assert _plan(FWD, 200704, 128) == SELECTION[(FWD, 200704, 128, 0, 0)]
    assert _plan(FWD, 97, 96, cus=2) == "cnblock_mlp_fwd_kernel" + tail.split(" grid=")[0] + (
        f" grid=1 block={64 * res} lds=150528 nt=0 tiles=4" if res in (8, 12) else
        " grid=1 block=768 lds=150528 nt=0 tiles=4" if res is None else " grid=1 block=256 lds=52224 nt=0 tiles=1")


FIRST = {0: "<96, 1, 8, 0>", 1: "<96, 1, 8, 1>", 2: "<96, 1, 8, 2>", 3: "<96, 1, 8, 0>", None: "<96, 1, 8, 2>"}


@pytest.mark.parametrize("w12", [0, 1])
@pytest.mark.parametrize("hto", [0, 1, 5, None])
@pytest.mark.parametrize("var", [0, 1, 2, 3, None])
def test_bwdw_knobs(var, hto, w12, monkeypatch):
    """MMG_BWDW_VAR 1 / 2, anything else 0; MMG_BWDW_HTO zero or not; MMG_BWDW_W12: launch 1 on 12 waves, which exists with schedule 0
    only - whatever MMG_BWDW_VAR says."""
    _set_env(monkeypatch, dict(DEFAULT, MMG_BWDW_VAR=var, MMG_BWDW_HTO=hto, MMG_BWDW_W12=w12))
    first = "<96, 1, 12, 0>" if w12 else FIRST[var]
    second = "<96, 2, 8, 0>" if hto == 0 else "<96, 2, 8, 1>"
    assert _plan(BWDW, 640, 96, cus=4) == f"cnblock_bwdw_kernel{first} + {second} grid=4 block=({768 if w12 else 512},512) lds=156032 nt=0 tiles=10"


REJECTED = [
    ((FWD, 64, 768), "mmg_cnblock_mlp_fwd: C=768 not in {96,128,192,256,384,512}"),
    ((FWD, 0, 96), "mmg_cnblock_mlp_fwd: bad M=0"),
    ((FWD, 1 << 36, 96), f"mmg_cnblock_mlp_fwd: bad M={1 << 36}"),
    ((BWD, 64, 256), "mmg_cnblock_mlp_bwd: C=256 not in {96,128,192,384}"),
    ((BWD, 64, 512), "mmg_cnblock_mlp_bwd: C=512 not in {96,128,192,384}"),
    ((BWD, 0, 384), "mmg_cnblock_mlp_bwd: bad M=0"),
    ((BWDW, 64, 192), "mmg_cnblock_bwdw: C=192 is not supported (96)"),
    ((BWDW, 65, 96), "mmg_cnblock_bwdw: M=65 must be a positive multiple of 64"),
    ((BWDW, 0, 96), "mmg_cnblock_bwdw: M=0 must be a positive multiple of 64"),
    ((BWDW, 22369664, 96), "mmg_cnblock_bwdw: M=22369664 rows exceed the 4 GiB buffer range of one launch"),
]


@pytest.mark.parametrize("args,message", REJECTED, ids=lambda v: v if isinstance(v, str) else None)
def test_rejected_shapes_give_no_plan_and_the_entry_points_message(args, message):
    lib = _hip.load()
    assert _plan(*args) == ""
    assert lib.mmg_last_error().decode() == message


def test_the_last_accepted_row_counts():
    assert 22369600 * 96 * 2 < 2 ** 32 <= 22369664 * 96 * 2
    assert _plan(BWDW, 22369600, 96).endswith(" tiles=349525")
    assert _plan(FWD, (1 << 36) - 1, 128).endswith(f" tiles={1 << 29}")


@pytest.mark.parametrize("args", [(3, 64, 96, 0, 0, 256), (-1, 64, 96, 0, 0, 256), (1, 64, 96, 1, 0, 256), (2, 64, 96, 0, 1, 256), (0, 64, 96, 0, 0, -1)])
def test_unknown_op_or_mode_gives_no_plan(args):
    lib = _hip.load()
    assert _plan(*args) == "" and lib.mmg_last_error().decode().startswith("mmg_cnblock_plan:")


def test_capability_helpers_agree_with_the_plan_and_with_the_rules_they_used_to_restate(monkeypatch):
    _set_env(monkeypatch, DEFAULT)
    lib = _hip.load()
    for C in range(32, 1025, 32):
        assert K.cnblock_supported(C) == bool(_plan(FWD, 64, C)) == (C in R.WIDTHS), C
        assert bool(lib.mmg_cnblock_packed_elems(C, 0)) == (C in R.WIDTHS), C
        assert bool(_plan(BWD, 64, C, cus=304)) == (K.cnblock_bwd_mode(C) != 0) == (C in R.BWD_WIDTHS), C
        for M in (1, 63, 64, 65, 128, 22369600, 22369664):
            want = C == 96 and M % 64 == 0 and M * C * 2 < 2 ** 32
            assert K.cnblock_bwdw_supported(C, M) == bool(_plan(BWDW, M, C)) == want, (C, M)
    assert lib.mmg_cnblock_bwdw_packed_elems(96) == 12 * 392 * 8 + 2 * 24 * 3 * 64 * 8 and lib.mmg_cnblock_bwdw_packed_elems(192) == 0
