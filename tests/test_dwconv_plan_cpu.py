"""The depthwise 7x7 host layer's plans (csrc/dwconv_plan.hip), read through mmg_dwconv7_plan with the CU count given: no GPU, nothing is
launched.

What a plan string holds: the kernel instantiation as mmg_last_kernel() spells it, then " grid=(x,y,z) block=T lds=B nt=0|1 tile=HxW
items=N" and, for the matrix-core door, " add=0|1 by_image=0|1".  The plans are compared with three things that do not come from the code
under test: the Python restatement of the launchers' rules (dwconv_ref.plan_text), the kernels the launchers BEFORE this host layer noted
on an MI355X for every case of dwconv_ref.CASES (profiles/dwconv_measured_tolerances.jsonl), and a literal table at the towers' own shapes."""
import json
import os
import re

import pytest

from mmgclip import _hip
from tests import dwconv_ref as R

RECORDS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dwconv_measured_tolerances.jsonl")
KNOBS = ("MMG_DWCONV_ROWS2", "MMG_DWCONV_TH", "MMG_DWG_TH", "MMG_DWG_ALIGN", "MMG_DWM_WAVES")
DEFAULT = dict.fromkeys(KNOBS)
NHWC, MFMA, WGRAD = 0, 1, 2
DOORS = ("mmg_dwconv7_nhwc", "mmg_dwconv7_nhwc_mfma", "mmg_dwconv7_wgrad")
PTR = 0x1000            # stands for a device pointer: validation compares pointers with NULL and never dereferences them

# (op, n, H, W, C, flip, add) -> plan on 256 CUs under default knobs.  64 images of 224 x 224: the depthwise maps of ConvNeXt-T (56^2 x 96,
# 28^2 x 192, 14^2 x 384, 7^2 x 768) and ConvNeXt-B (128 / 256 / 512 / 1024), and 64 maps of 256^2 x 96, where the matrix cores are the
# default.  Each line worked out by hand from the launchers before this host layer:
#   op 0  tiles of 8 x 32: grid = (ceil(W / 32) ceil(H / 8), C / 32, n); lds = 14 rows x 616 dwords x 4 + 49 x 32 x 4 = 34 496 + 6 272
#   op 1  tiles of 16 x 16; grid = 8 max(256 / 8, C / 32) unless ceil(items / 8) C / 32 is smaller (never here: at 7^2 x 768 it is
#         8 x 24 = 192 >= 32); block = 16 waves; lds = 32 768 + 32 x 2 128 + 20 480 = 121 344, + 20 480 with add
#   op 2  16-row tiles iff n ceil(H / 16) ceil(W / 32) C / 32 >= 2048: 56^2 x 96 -> 64 x 4 x 2 x 3 = 1536 (8), 56^2 x 128 -> 2048 (16),
#         7^2 x 768 -> 1536 (8), 7^2 x 1024 -> 2048 (16), 256^2 x 96 -> 24 576 (16), the others 768 / 1024 (8);
#         grid.x = 1024 / (C / 32) rounded down to a multiple of 8 (341 -> 336, 170 -> 168, 85 -> 80, 42 -> 40), never above n x tiles;
#         lds = (TH + 6) x 616 x 4 + 4 x 50 x 32 x 4 = 34 496 (54 208 at TH = 16) + 25 600
#   nt    n H W C x 2 bytes >= 268 435 456: only 64 x 256^2 x 96 x 2 = 805 306 368; never the weight gradient
SELECTION = {
    (NHWC, 64, 56, 56, 96, 0, 0): "dwconv7_rows2_kernel<false, 8> grid=(14,3,64) block=256 lds=40768 nt=0 tile=8x32 items=896",
    (NHWC, 64, 56, 56, 96, 1, 1): "dwconv7_rows2_kernel<true, 8> grid=(14,3,64) block=256 lds=40768 nt=0 tile=8x32 items=896",
    (NHWC, 64, 28, 28, 192, 0, 0): "dwconv7_rows2_kernel<false, 8> grid=(4,6,64) block=256 lds=40768 nt=0 tile=8x32 items=256",
    (NHWC, 64, 28, 28, 192, 1, 1): "dwconv7_rows2_kernel<true, 8> grid=(4,6,64) block=256 lds=40768 nt=0 tile=8x32 items=256",
    (NHWC, 64, 14, 14, 384, 0, 0): "dwconv7_rows2_kernel<false, 8> grid=(2,12,64) block=256 lds=40768 nt=0 tile=8x32 items=128",
    (NHWC, 64, 14, 14, 384, 1, 0): "dwconv7_rows2_kernel<true, 8> grid=(2,12,64) block=256 lds=40768 nt=0 tile=8x32 items=128",
    (NHWC, 64, 7, 7, 768, 0, 0): "dwconv7_rows2_kernel<false, 8> grid=(1,24,64) block=256 lds=40768 nt=0 tile=8x32 items=64",
    (NHWC, 64, 7, 7, 768, 0, 1): "dwconv7_rows2_kernel<false, 8> grid=(1,24,64) block=256 lds=40768 nt=0 tile=8x32 items=64",
    (NHWC, 64, 56, 56, 128, 0, 0): "dwconv7_rows2_kernel<false, 8> grid=(14,4,64) block=256 lds=40768 nt=0 tile=8x32 items=896",
    (NHWC, 64, 28, 28, 256, 1, 1): "dwconv7_rows2_kernel<true, 8> grid=(4,8,64) block=256 lds=40768 nt=0 tile=8x32 items=256",
    (NHWC, 64, 14, 14, 512, 0, 0): "dwconv7_rows2_kernel<false, 8> grid=(2,16,64) block=256 lds=40768 nt=0 tile=8x32 items=128",
    (NHWC, 64, 7, 7, 1024, 1, 1): "dwconv7_rows2_kernel<true, 8> grid=(1,32,64) block=256 lds=40768 nt=0 tile=8x32 items=64",
    (NHWC, 64, 256, 256, 96, 0, 0): "dwconv7_rows2_kernel<false, 8> grid=(256,3,64) block=256 lds=40768 nt=1 tile=8x32 items=16384",
    (MFMA, 64, 56, 56, 96, 0, 0): "dwconv7_mfma_kernel<false, 16> grid=(256,1,1) block=1024 lds=121344 nt=0 tile=16x16 items=1024 add=0 by_image=1",
    (MFMA, 64, 56, 56, 96, 1, 1): "dwconv7_mfma_kernel<true, 16> grid=(256,1,1) block=1024 lds=141824 nt=0 tile=16x16 items=1024 add=1 by_image=1",
    (MFMA, 64, 28, 28, 192, 0, 0): "dwconv7_mfma_kernel<false, 16> grid=(256,1,1) block=1024 lds=121344 nt=0 tile=16x16 items=256 add=0 by_image=1",
    (MFMA, 64, 14, 14, 384, 1, 1): "dwconv7_mfma_kernel<true, 16> grid=(256,1,1) block=1024 lds=141824 nt=0 tile=16x16 items=64 add=1 by_image=1",
    (MFMA, 64, 7, 7, 768, 0, 0): "dwconv7_mfma_kernel<false, 16> grid=(256,1,1) block=1024 lds=121344 nt=0 tile=16x16 items=64 add=0 by_image=1",
    (MFMA, 64, 56, 56, 128, 1, 1): "dwconv7_mfma_kernel<true, 16> grid=(256,1,1) block=1024 lds=141824 nt=0 tile=16x16 items=1024 add=1 by_image=1",
    (MFMA, 64, 28, 28, 256, 0, 0): "dwconv7_mfma_kernel<false, 16> grid=(256,1,1) block=1024 lds=121344 nt=0 tile=16x16 items=256 add=0 by_image=1",
    (MFMA, 64, 14, 14, 512, 0, 0): "dwconv7_mfma_kernel<false, 16> grid=(256,1,1) block=1024 lds=121344 nt=0 tile=16x16 items=64 add=0 by_image=1",
    (MFMA, 64, 7, 7, 1024, 1, 1): "dwconv7_mfma_kernel<true, 16> grid=(256,1,1) block=1024 lds=141824 nt=0 tile=16x16 items=64 add=1 by_image=1",
    (MFMA, 64, 256, 256, 96, 0, 0): "dwconv7_mfma_kernel<false, 16> grid=(256,1,1) block=1024 lds=121344 nt=1 tile=16x16 items=16384 add=0 by_image=1",
    (MFMA, 64, 256, 256, 96, 0, 1): "dwconv7_mfma_kernel<false, 16> grid=(256,1,1) block=1024 lds=141824 nt=1 tile=16x16 items=16384 add=1 by_image=1",
    (MFMA, 64, 256, 256, 96, 1, 0): "dwconv7_mfma_kernel<true, 16> grid=(256,1,1) block=1024 lds=121344 nt=1 tile=16x16 items=16384 add=0 by_image=1",
    (MFMA, 64, 256, 256, 96, 1, 1): "dwconv7_mfma_kernel<true, 16> grid=(256,1,1) block=1024 lds=141824 nt=1 tile=16x16 items=16384 add=1 by_image=1",
    (WGRAD, 64, 56, 56, 96, 0, 0): "dwconv7_wgrad_rows2_kernel<8> grid=(336,3,1) block=256 lds=60096 nt=0 tile=8x32 items=896",
    (WGRAD, 64, 28, 28, 192, 0, 0): "dwconv7_wgrad_rows2_kernel<8> grid=(168,6,1) block=256 lds=60096 nt=0 tile=8x32 items=256",
    (WGRAD, 64, 14, 14, 384, 0, 0): "dwconv7_wgrad_rows2_kernel<8> grid=(80,12,1) block=256 lds=60096 nt=0 tile=8x32 items=128",
    (WGRAD, 64, 7, 7, 768, 0, 0): "dwconv7_wgrad_rows2_kernel<8> grid=(40,24,1) block=256 lds=60096 nt=0 tile=8x32 items=64",
    (WGRAD, 64, 56, 56, 128, 0, 0): "dwconv7_wgrad_rows2_kernel<16> grid=(256,4,1) block=256 lds=79808 nt=0 tile=16x32 items=512",
    (WGRAD, 64, 28, 28, 256, 0, 0): "dwconv7_wgrad_rows2_kernel<8> grid=(128,8,1) block=256 lds=60096 nt=0 tile=8x32 items=256",
    (WGRAD, 64, 14, 14, 512, 0, 0): "dwconv7_wgrad_rows2_kernel<8> grid=(64,16,1) block=256 lds=60096 nt=0 tile=8x32 items=128",
    (WGRAD, 64, 7, 7, 1024, 0, 0): "dwconv7_wgrad_rows2_kernel<16> grid=(32,32,1) block=256 lds=79808 nt=0 tile=16x32 items=64",
    (WGRAD, 64, 256, 256, 96, 0, 0): "dwconv7_wgrad_rows2_kernel<16> grid=(336,3,1) block=256 lds=79808 nt=0 tile=16x32 items=8192",
}
TEXT = re.compile(r"(?P<kernel>\S+(?:<[^>]*>)?) grid=\((?P<gx>\d+),(?P<gy>\d+),(?P<gz>\d+)\) block=(?P<block>\d+) lds=(?P<lds>\d+) nt=(?P<nt>[01])"
                  r" tile=(?P<th>\d+)x(?P<tw>\d+) items=(?P<items>\d+)(?: add=(?P<add>[01]) by_image=(?P<by_image>[01]))?")


def _set_env(monkeypatch, env):
    for name, v in env.items():
        if name not in KNOBS:                # (MMG_DWCONV_MFMA picks the door in Python: here the op does)
            continue
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _plan(op, n, H, W, C, flip=0, add=0, cus=256):
    return _hip.load().mmg_dwconv7_plan(op, n, H, W, C, flip, add, cus).decode()


def _fields(text):
    m = TEXT.fullmatch(text)
    assert m, text
    return {k: (v if k == "kernel" else None if v is None else int(v)) for k, v in m.groupdict().items()}


def _kernel(text):
    return text.split(" grid=")[0]


def _case(op, n, H, W, C, flip=0, add=0, **knobs):
    return R.Case(n, H, W, C, "integer", "wgrad" if op == WGRAD else "conv", int(op == MFMA), flip=bool(flip), add=bool(add), **knobs)


def _recorded():
    """test id -> the kernels noted on the device by the launchers before the plan existed (a case was recorded more than once)."""
    out = {}
    with open(RECORDS) as f:
        for r in map(json.loads, f):
            if r["test"].startswith("dwconv_f64_") and "kernel" in r:
                out.setdefault(r["test"].split("@")[0], set()).add(r["kernel"])      # ("...@parent": the same launch, an earlier kernel)
    return out


RECORDED = _recorded()
BY_ID = {"dwconv_f64_" + c.id: c for c in R.CASES}


@pytest.mark.parametrize("cus", [2, 256, 304])
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_plan_is_the_restated_one(case, cus, monkeypatch):
    _set_env(monkeypatch, dict(DEFAULT, **case.env))
    assert _plan(*R.plan_args(case, cus)) == R.plan_text(case, cus)


@pytest.mark.parametrize("test", sorted(RECORDED))
def test_plan_names_the_kernel_of_the_recorded_launch(test, monkeypatch):
    assert test in BY_ID, f"{test}: a recorded launch without a case in dwconv_ref.CASES"
    case = BY_ID[test]
    _set_env(monkeypatch, dict(DEFAULT, **case.env))
    assert {_kernel(_plan(*R.plan_args(case, 256)))} == RECORDED[test]


def test_every_case_has_a_recorded_launch():
    assert not [t for t in BY_ID if t not in RECORDED]


def test_the_table_names_exactly_the_built_kernels(monkeypatch):
    """Over the cases: the notes of the 17 instantiations of dwconv_ref.ALL_INSTANTIATIONS (the matrix-core note does not spell ADD, the
    plan's add field does), no other."""
    assert len(R.ALL_INSTANTIATIONS) == 17
    seen = set()
    for case in R.CASES:
        _set_env(monkeypatch, dict(DEFAULT, **case.env))
        f = _fields(_plan(*R.plan_args(case, 256)))
        assert f["kernel"] == R.kernel_note(case)
        seen.add(R.instantiations(case)[0][:3] + ((bool(f["add"]),) if f["add"] is not None else ()))
    assert seen == R.ALL_INSTANTIATIONS


def test_selection_table(monkeypatch):
    """The literals against the library and against the restatement; every tower shape, the three ops, both flips, with and without add."""
    _set_env(monkeypatch, DEFAULT)
    wrong = {s: (_plan(*s), want) for s, want in SELECTION.items() if _plan(*s) != want}
    assert not wrong, wrong
    for s, want in SELECTION.items():
        assert want == R.plan_text(_case(*s), 256), s
    shapes = {(56, 96), (28, 192), (14, 384), (7, 768), (56, 128), (28, 256), (14, 512), (7, 1024), (256, 96)}
    for op in (NHWC, MFMA, WGRAD):
        assert {(s[2], s[4]) for s in SELECTION if s[0] == op} == shapes
    assert {s[5:] for s in SELECTION if s[0] == NHWC} == {s[5:] for s in SELECTION if s[0] == MFMA} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_streaming_stores_from_256_mib(monkeypatch):
    """n H W C x 2 bytes >= 2^28: 64 x 256 x 256 x 32 x 2 is exactly 2^28; one row less is below.  Both forward doors; never the weight gradient."""
    _set_env(monkeypatch, DEFAULT)
    assert 64 * 256 * 256 * 32 * 2 == 256 << 20
    for op in (NHWC, MFMA):
        assert _fields(_plan(op, 64, 256, 256, 32))["nt"] == 1 and _fields(_plan(op, 64, 255, 256, 32))["nt"] == 0
        assert _fields(_plan(op, 64, 256, 256, 32, 1, 1))["nt"] == 1 and _fields(_plan(op, 63, 256, 256, 32, 1, 1))["nt"] == 0
    assert _fields(_plan(WGRAD, 64, 256, 256, 32))["nt"] == 0 and _fields(_plan(WGRAD, 64, 256, 256, 96))["nt"] == 0


def test_wgrad_tile_height_rule(monkeypatch):
    """16 rows iff n ceil(H / 16) ceil(W / 32) C / 32 >= 2048: 64 x 4 x 2 x 4 = 2048, 63 x 4 x 2 x 4 = 2016; a 17th row makes a 5th tile row
    only at ceil(H / 16): 51 x 5 x 2 x 4 = 2040, 52 x 5 x 2 x 4 = 2080."""
    _set_env(monkeypatch, DEFAULT)
    th = lambda *s: _fields(_plan(WGRAD, *s))["th"]
    assert (th(64, 56, 56, 128), th(63, 56, 56, 128)) == (16, 8)
    assert (th(52, 65, 56, 128), th(51, 65, 56, 128), th(51, 65, 65, 128)) == (16, 8, 16)
    assert (th(1, 16, 32, 32 * 2048), th(1, 16, 32, 32 * 2047)) == (16, 8)


def test_wgrad_workgroups_per_slab(monkeypatch):
    """1024 / slabs, down to a multiple of 8 from 8 up (MMG_DWG_ALIGN, read on EVERY call), at least 1, at most n x tiles."""
    _set_env(monkeypatch, DEFAULT)
    gx = lambda *s: _fields(_plan(WGRAD, *s))["gx"]
    big = (128, 56, 56)                                 # 1792 items of 8 rows, 1024 of 16: no cap below
    assert gx(*big, 96) == 336 and gx(*big, 32) == 1024 and gx(*big, 32 * 128) == 8              # 341 -> 336; 1024; 8
    assert gx(*big, 32 * 129) == 7 and gx(*big, 32 * 200) == 5                                   # below 8: as they are
    assert gx(*big, 32 * 1024) == 1 and gx(*big, 32 * 1025) == 1                                 # 1024 / 1025 = 0 -> 1
    assert gx(2, 9, 33, 64) == 8 and gx(1, 1, 1, 32) == 1 and gx(1, 8, 33, 96) == 2              # capped by n x tiles (8, 1, 2)
    assert gx(3, 8, 33, 96) == 6 and gx(42, 8, 256, 96) == 336 and gx(41, 8, 256, 96) == 328    # 6 items; 336 items: not capped; 328: capped
    for v, want in (("0", 341), ("1", 336), ("0", 341), ("5", 336), ("-1", 336), ("x", 341)):    # per call; non-zero = on; atoi("x") = 0
        monkeypatch.setenv("MMG_DWG_ALIGN", v)
        assert gx(*big, 96) == want, v
        assert gx(*big, 32 * 200) == 5 and gx(2, 9, 33, 64) == 8
        assert _plan(WGRAD, *big, 96) == R.plan_text(_case(WGRAD, *big, 96), 256, align=want == 336)


def test_matrix_core_grid(monkeypatch):
    """8 max(cus / 8, slabs), capped by ceil(items / 8) slabs; a multiple of 8 on any CU count."""
    _set_env(monkeypatch, DEFAULT)
    gx = lambda cus, *s: _fields(_plan(MFMA, *s, cus=cus))["gx"]
    assert gx(256, 64, 56, 56, 96) == 256 and gx(304, 64, 56, 56, 96) == 304 and gx(2, 64, 56, 56, 96) == 24 and gx(100, 64, 56, 56, 96) == 96
    assert gx(256, 8, 64, 64, 1280) == 320 and gx(304, 8, 64, 64, 1280) == 320               # cus / 8 = 32, 38 < 40 slabs; want = 16 x 40
    assert gx(256, 1, 16, 16, 32) == 8 and gx(256, 2, 3, 5, 64) == 16                        # 1 / 2 items: want = slabs
    assert gx(256, 9, 16, 16, 32) == 16 and gx(256, 1, 64, 70, 32) == 24                     # 9 items -> 2; 20 items -> 3
    assert gx(256, 1, 16, 16 * 255, 32) == 256 and gx(256, 1, 16, 16 * 249 - 15, 32) == 256 and gx(256, 1, 16, 16 * 248, 32) == 248
    for cus in (1, 2, 7, 8, 9, 104, 256, 304):
        for s in ((1, 1, 1, 32), (3, 37, 50, 96), (64, 56, 56, 96), (5, 250, 270, 32)):
            assert gx(cus, *s) == R.mfma_plan(*s, cus)["grid"] and gx(cus, *s) % 8 == 0


def test_by_image_from_eight_images(monkeypatch):
    _set_env(monkeypatch, DEFAULT)
    assert [_fields(_plan(MFMA, n, 20, 35, 32))["by_image"] for n in (1, 7, 8, 9)] == [0, 0, 1, 1]
    assert _fields(_plan(NHWC, 8, 20, 35, 32))["by_image"] is None


# knob -> (values, what they select); None = unset.  Out-of-range values fall back as the launchers before this host layer did.
@pytest.mark.parametrize("rows2", [None, 1, 0, 7, -1])
@pytest.mark.parametrize("th", [None, 8, 16, 12, 0])
def test_forward_knobs(rows2, th, flip=1):
    """MMG_DWCONV_ROWS2: zero or not; MMG_DWCONV_TH: 16, anything else 8 - and ignored by the one-row kernel (8 rows, its own LDS pitch)."""
    with pytest.MonkeyPatch.context() as mp:
        _set_env(mp, dict(DEFAULT, MMG_DWCONV_ROWS2=rows2, MMG_DWCONV_TH=th))
        text = _plan(NHWC, 3, 37, 50, 96, flip, 1)
        assert text == R.plan_text(_case(NHWC, 3, 37, 50, 96, flip, 1, rows2=rows2, th=th), 256)
    if rows2 == 0:
        assert text == "dwconv7_kernel<true> grid=(10,3,3) block=256 lds=41216 nt=0 tile=8x32 items=30"          # 14 x 624 x 4 + 6272
    elif th == 16:
        assert text == "dwconv7_rows2_kernel<true, 16> grid=(6,3,3) block=256 lds=60480 nt=0 tile=16x32 items=18"  # 22 x 616 x 4 + 6272
    else:
        assert text == "dwconv7_rows2_kernel<true, 8> grid=(10,3,3) block=256 lds=40768 nt=0 tile=8x32 items=30"


@pytest.mark.parametrize("rows2", [None, 1, 0, 7])
@pytest.mark.parametrize("gth", [None, 8, 16, 12, 0, -16])
def test_wgrad_knobs(rows2, gth):
    """MMG_DWG_TH: 8 / 16, anything else by rule (3 x 3 x 2 x 3 = 54 < 2048: 8) - and ignored by the one-row kernel."""
    with pytest.MonkeyPatch.context() as mp:
        _set_env(mp, dict(DEFAULT, MMG_DWCONV_ROWS2=rows2, MMG_DWG_TH=gth))
        text = _plan(WGRAD, 3, 37, 50, 96)
        assert text == R.plan_text(_case(WGRAD, 3, 37, 50, 96, rows2=rows2, gth=gth), 256)
    if rows2 == 0:
        assert text == "dwconv7_wgrad_kernel grid=(30,3,1) block=256 lds=60544 nt=0 tile=8x32 items=30"           # 14 x 624 x 4 + 25600
    elif gth == 16:
        assert text == "dwconv7_wgrad_rows2_kernel<16> grid=(18,3,1) block=256 lds=79808 nt=0 tile=16x32 items=18"
    else:
        assert text == "dwconv7_wgrad_rows2_kernel<8> grid=(30,3,1) block=256 lds=60096 nt=0 tile=8x32 items=30"


@pytest.mark.parametrize("waves", [None, 16, 8, 4, 0, 12])
@pytest.mark.parametrize("add", [0, 1])
def test_matrix_core_knob(waves, add):
    """MMG_DWM_WAVES: 8, anything else 16; the block is 64 threads per wave; LDS is the larger layout iff add is given."""
    with pytest.MonkeyPatch.context() as mp:
        _set_env(mp, dict(DEFAULT, MMG_DWM_WAVES=waves, MMG_DWCONV_ROWS2=0, MMG_DWCONV_TH=16))       # (the VALU knobs do not reach it)
        text = _plan(MFMA, 3, 37, 50, 96, 0, add)
        assert text == R.plan_text(_case(MFMA, 3, 37, 50, 96, 0, add, waves=waves), 256)
    nw = 8 if waves == 8 else 16
    assert text == (f"dwconv7_mfma_kernel<false, {nw}> grid=(120,1,1) block={64 * nw} lds={141824 if add else 121344} nt=0 tile=16x16 "
                    f"items=36 add={add} by_image=0")                                                # want = ceil(36 / 8) x 3 = 15 < 32


# ---- rejections: the plan door gives "" and the entry point's own message; the entry point itself returns before any HIP call ----
VALU_BAD = [
    ((2, 8, 32, 48), "n=2 H=8 W=32 C=48 (C must be a multiple of 32)"),
    ((0, 8, 32, 32), "n=0 H=8 W=32 C=32 (C must be a multiple of 32)"),
    ((2, 0, 32, 32), "n=2 H=0 W=32 C=32 (C must be a multiple of 32)"),
    ((2, 8, -1, 32), "n=2 H=8 W=-1 C=32 (C must be a multiple of 32)"),
    ((2, 8, 32, 0), "n=2 H=8 W=32 C=0 (C must be a multiple of 32)"),
    ((65536, 8, 32, 32), "n=65536 H=8 W=32 C=32 (C must be a multiple of 32)"),
    ((1, 1, 1, 32 * 65536), "n=1 H=1 W=1 C=2097152 (C must be a multiple of 32)"),
    # 24-bit pixel indices: (H + 16) (W + 64) <= 2^24 holds at 4080 x 4032 (4096 x 4096) and not one row further
    ((1, 4081, 4032, 32), "one image of 4081 x 4032 x 32 exceeds the kernels' 32-bit addressing (H * W <= 2^24, H * W * C * 2 < 2^32)"),
    # 32-bit byte offsets: 1024 x 1024 x C x 2 < 2^32 holds up to C = 2047
    ((1, 1024, 1024, 2048), "one image of 1024 x 1024 x 2048 exceeds the kernels' 32-bit addressing (H * W <= 2^24, H * W * C * 2 < 2^32)"),
]
MFMA_BAD = [(s, m) for s, m in VALU_BAD[:5]] + [
    # int offsets inside a tile's band of rows: min(H, 22) W C < 2^31.  22 x 1024 x 95 328 = 2^31 + 65 536; one row: 1024 x 2^21 = 2^31
    ((1, 22, 1024, 95328), "22 rows of 1024 x 95328 exceed the kernel's 32-bit offsets inside a tile (min(H, 22) * W * C < 2^31)"),
    ((1, 4000, 1024, 95328), "22 rows of 1024 x 95328 exceed the kernel's 32-bit offsets inside a tile (min(H, 22) * W * C < 2^31)"),
    ((1, 1, 1024, 1 << 21), "1 rows of 1024 x 2097152 exceed the kernel's 32-bit offsets inside a tile (min(H, 22) * W * C < 2^31)"),
    ((1 << 20, 512, 512, 32), "too many tiles"),                     # 2^20 x 32 x 32 = 2^30 items
    ((1, 1 << 19, 1 << 19, 32), "too many tiles"),                   # 2^15 x 2^15 tiles per image
]
REJECTED = [(op, s, m) for op in (NHWC, WGRAD) for s, m in VALU_BAD] + [(MFMA, s, m) for s, m in MFMA_BAD]


def _call(op, shape, null=None, flip=0):
    """The real entry point with stand-in pointers (`null`: that operand missing) -> its return code."""
    lib, name = _hip.load(), DOORS[op]
    names = _hip.parse_header()[name][2]
    given = dict(zip(("n", "H", "W", "C"), shape), flip=flip, stream=None, bias=None, add=None, dbias=None)
    given[null] = None
    return getattr(lib, name)(*[given.get(a, PTR) for a in names])


@pytest.mark.parametrize("op,shape,message", REJECTED, ids=[f"{DOORS[op]}-{'x'.join(map(str, s))}" for op, s, _ in REJECTED])
def test_rejected_shapes_give_no_plan_and_the_entry_points_message(op, shape, message):
    lib = _hip.load()
    assert _plan(op, *shape) == ""
    assert lib.mmg_last_error().decode() == f"{DOORS[op]}: {message}"
    lib.mmg_dwconv7_plan(op, 2, 8, 32, 32, 0, 0, 256)
    assert _call(op, shape) != 0
    assert lib.mmg_last_error().decode() == f"{DOORS[op]}: {message}"


@pytest.mark.parametrize("op,null", [(NHWC, "x"), (NHWC, "w"), (NHWC, "y"), (MFMA, "x"), (MFMA, "w"), (MFMA, "y"),
                                     (WGRAD, "x"), (WGRAD, "dy"), (WGRAD, "dw")])
def test_null_operands_are_rejected_before_any_launch(op, null):
    assert _call(op, (2, 8, 32, 32), null=null) != 0
    assert _hip.load().mmg_last_error().decode() == f"{DOORS[op]}: null pointer"


def test_the_last_accepted_shapes(monkeypatch):
    """The other side of every bound; what only the VALU doors bound, the matrix-core door takes."""
    _set_env(monkeypatch, DEFAULT)
    for op in (NHWC, WGRAD):
        assert _fields(_plan(op, 65535, 8, 32, 32))["items"] == 65535
        assert _fields(_plan(op, 1, 1, 1, 32 * 65535))["gy"] == 65535
        assert _fields(_plan(op, 1, 4080, 4032, 32))["items"] == (510 if op == NHWC else 255) * 126      # (weight gradient: 16-row tiles)
        assert (4080 + 16) * (4032 + 64) == 1 << 24 and 1024 * 1024 * 2016 * 2 < 1 << 32 <= 1024 * 1024 * 2048 * 2
        assert _fields(_plan(op, 1, 1024, 1024, 2016))["gy"] == 63
    assert _fields(_plan(MFMA, 65536, 8, 32, 32))["items"] == 65536 * 2
    assert _plan(MFMA, 1, 4081, 4032, 32) and _plan(MFMA, 1, 1024, 1024, 2048)
    assert 22 * 1024 * 95296 < 1 << 31 < 22 * 1024 * 95328
    assert _plan(MFMA, 1, 22, 1024, 95296) and _plan(MFMA, 1, 4000, 1024, 95296) and _plan(MFMA, 1, 1, 1024, (1 << 21) - 32)
    assert _fields(_plan(MFMA, (1 << 20) - 1, 512, 512, 32))["items"] == (1 << 30) - 1024


@pytest.mark.parametrize("args", [(3, 2, 8, 32, 32, 0, 0, 256), (-1, 2, 8, 32, 32, 0, 0, 256), (2, 2, 8, 32, 32, 1, 0, 256),
                                  (2, 2, 8, 32, 32, 0, 1, 256), (0, 2, 8, 32, 32, 0, 0, -1)])
def test_unknown_op_or_mode_gives_no_plan(args):
    lib = _hip.load()
    assert _plan(*args) == "" and lib.mmg_last_error().decode().startswith("mmg_dwconv7_plan:")


def test_invariants_over_a_grid_of_shapes(monkeypatch):
    """Every dimension of every grid at least 1, LDS inside the CU's 160 KiB, the matrix-core grid a multiple of 8 whose streams, as
    the kernel deals them (dwconv_ref.mfma_plan), take every (image, tile) item of every slab exactly once."""
    _set_env(monkeypatch, DEFAULT)
    for n in (1, 7, 8, 9, 64):
        for H, W in ((1, 1), (7, 7), (16, 16), (17, 33), (56, 56), (37, 250)):
            for C in (32, 96, 1024):
                for cus in (2, 256, 304):
                    for op in (NHWC, MFMA, WGRAD):
                        f = _fields(_plan(op, n, H, W, C, cus=cus))
                        assert min(f["gx"], f["gy"], f["gz"]) >= 1 and 0 < f["lds"] <= 160 * 1024 and f["block"] in (256, 512, 1024), f
                        assert f["items"] == n * R.cdiv(H, f["th"]) * R.cdiv(W, f["tw"]), f
                        if op == MFMA:
                            deal = R.mfma_plan(n, H, W, C, cus)
                            assert f["gx"] % 8 == 0 and f["gx"] == deal["grid"] and (f["gy"], f["gz"]) == (1, 1), f
                            assert deal["slab_items"] == [f["items"]] * (C // 32), (f, deal)
                        elif op == WGRAD:
                            assert f["gx"] <= f["items"] and f["gy"] == C // 32, f
                        else:
                            assert f["gx"] * f["gz"] == f["items"] and f["gy"] == C // 32, f
