"""The case table, the exact-data regimes and the bars of tests/dwconv_ref.py, checked without a GPU on every row the GPU tests run:
the table reaches every template instantiation of csrc/dwconv7.hip and csrc/dwconv7_mfma.hip, both walks and both halo paths of the
matrix-core kernel and both item loops; a bar of zero is justified for every integer and read-out case by the float64 reference
alone; a tile-by-tile emulation of the kernels (float64 with their rounding points) is inside every bar; and every mutation of it -
a dropped tap, a shifted halo, replicate padding, the previous item's zero mask, unflipped taps, exchanged channel pairs, a lost add,
an unwritten row, a skipped image, a tile index off by one, a missing item / pass, dbias over the image edge - leaves the bar in every
case that contains the feature.  This is how the GPU tests are known to fail for a subtly wrong kernel."""
import pytest
import torch

from tests import dwconv_ref as R

CONV = [c for c in R.CASES if c.op == "conv"]
WGRAD = [c for c in R.CASES if c.op == "wgrad"]
BIG = 2_000_000        # cases above this many elements are emulated on image 0 only (the item loops' walk is checked by the plan tests)


def test_case_ids_are_unique_and_the_table_reaches_every_instantiation_in_an_exact_regime():
    assert len({c.id for c in R.CASES}) == len(R.CASES)
    # dwconv7_kernel<FLIP> 2, dwconv7_rows2_kernel<FLIP, 8|16> 4, dwconv7_mfma_kernel<FLIP, 8|16, ADD> 8, dwconv7_wgrad_kernel 1,
    # dwconv7_wgrad_rows2_kernel<8|16> 2: seventeen (every instantiation the two launchers can reach)
    assert len(R.ALL_INSTANTIATIONS) == 17
    seen = {}
    for c in R.CASES:
        for inst in R.instantiations(c):
            seen.setdefault(inst, set()).add(c.regime)
    assert set(seen) == R.ALL_INSTANTIATIONS, R.ALL_INSTANTIATIONS ^ set(seen)
    for inst, regimes in seen.items():
        assert "integer" in regimes, inst
    # all four add x flip combinations on both forward families, bias / dbias given and not
    for mfma in (0, 1):
        assert {(c.add, c.flip) for c in CONV if c.mfma == mfma and c.regime == "integer"} == {(a, f) for a in (0, 1) for f in (0, 1)}
        assert {c.bias for c in CONV if c.mfma == mfma and c.regime == "integer"} == {True, False}
    assert {c.bias for c in WGRAD} == {True, False}
    # every regime on every entry point
    for sel in (lambda c: c.op == "conv" and not c.mfma, lambda c: c.op == "conv" and c.mfma, lambda c: c.op == "wgrad"):
        assert {c.regime for c in R.CASES if sel(c)} == {"integer", "readout", "gaussian"}
    assert all(c.n * c.H * c.W * c.C <= 12_000_000 and c.C % 32 == 0 for c in R.CASES)
    # read-out needs every tap: C >= 49 (cases 2x3x5x64, 1x7x7x96, 1x9x33x64, 1x17x17x64, 3x37x50x96)
    assert all(c.C >= 49 for c in R.CASES if c.regime == "readout" and c.op == "conv")
    assert sorted({R.readout_tap(c) for c in range(49)}) == list(range(49))


def test_the_required_geometries_are_in_the_table():
    shapes = {(c.n, c.H, c.W, c.C) for c in R.CASES}
    assert {(1, 1, 1, 32), (2, 3, 5, 64), (1, 7, 7, 96), (2, 8, 32, 32), (1, 9, 33, 64), (2, 16, 32, 32), (1, 17, 33, 32), (2, 16, 16, 32),
            (1, 17, 17, 64), (3, 37, 50, 96), (9, 20, 35, 32), (5, 250, 270, 32), (3, 170, 180, 128), (12, 9, 97, 1024)} <= shapes
    valu = {(c.n, c.H, c.W, c.C): set() for c in CONV}
    for c in CONV:
        valu[(c.n, c.H, c.W, c.C)].add("mfma" if c.mfma else R.tile_hw(c)[0])
    for s in ((2, 8, 32, 32), (1, 9, 33, 64)):
        assert 8 in valu[s]
    for s in ((2, 16, 32, 32), (1, 17, 33, 32)):
        assert 16 in valu[s]
    for s in ((2, 16, 16, 32), (1, 17, 17, 64), (1, 1, 1, 32), (2, 3, 5, 64), (1, 7, 7, 96), (3, 37, 50, 96)):
        assert "mfma" in valu[s]


def test_the_matrix_core_cases_cover_both_walks_both_halo_paths_and_the_item_loop():
    mf = [c for c in CONV if c.mfma]
    assert {c.n >= 8 for c in mf} == {True, False}
    for by_image in (True, False):
        assert any(c.regime == "integer" for c in mf if (c.n >= 8) == by_image)
    paths = set().union(*(R.mfma_halo_paths(c.H, c.W) for c in mf if c.regime == "integer"))
    assert paths == {True, False}
    assert any(c.H >= 51 and c.W >= 51 and True in R.mfma_halo_paths(c.H, c.W) for c in mf)
    assert R.mfma_halo_paths(20, 35) == {False} and R.mfma_halo_paths(37, 50) == R.mfma_halo_paths(64, 70) == {True, False}
    # by image: 9 % 8 != 0 - XCD group 0 walks two images (12 items over 7 streams), the others one (6 items: their seventh stream idles)
    p = R.mfma_plan(9, 20, 35, 32, 256)
    assert p["by_image"] and (p["per_img"], p["grid"], p["min_items"], p["max_items"]) == (6, 56, 0, 2)
    # the item loop at n < 8 on 256 CUs: at least 5 items per stream (the prefetch of item + 2 and both parities at work), and the tiles of
    # an image are no multiple of the stream stride, so a stream's items move over the map
    loops = [c for c in mf if c.n < 8 and R.mfma_plan(c.n, c.H, c.W, c.C, 256)["min_items"] >= 5]
    assert {(c.n, c.H, c.W, c.C) for c in loops} == {(5, 250, 270, 32), (3, 170, 180, 128)}
    p = R.mfma_plan(5, 250, 270, 32, 256)
    assert (p["items"], p["grid"], p["min_items"], p["max_items"], p["strides"]) == (1360, 256, 5, 6, {256})
    p = R.mfma_plan(3, 170, 180, 128, 256)
    assert (p["items"], p["grid"], p["slabs"], p["min_items"], p["max_items"], p["strides"]) == (396, 256, 4, 6, 7, {64})
    for c in loops:
        p = R.mfma_plan(c.n, c.H, c.W, c.C, 256)
        assert all(p["per_img"] % s != 0 for s in p["strides"]) and c.regime == "integer"
        assert R.mfma_halo_paths(c.H, c.W) == {True, False}
    # every other case gives a stream at most two items off the by-image branch (what the older tests reached)
    assert {c.waves for c in loops} == {None, 8}


def test_the_weight_gradient_cases_run_the_item_loop_on_every_kernel():
    plans = {c.id: R.wgrad_plan(c) for c in WGRAD}
    loop = [c for c in WGRAD if plans[c.id]["min_items"] >= 3]
    assert {R.instantiations(c)[0] for c in loop} == {("dwconv7_wgrad_kernel",), ("dwconv7_wgrad_rows2_kernel", 8),
                                                      ("dwconv7_wgrad_rows2_kernel", 16)}
    assert {c.regime for c in loop} == {"integer", "gaussian"}
    big = [c for c in WGRAD if (c.n, c.H, c.W, c.C) == (12, 9, 97, 1024)]
    assert {(c.rows2, c.gth) for c in big} == {(None, 8), (None, 16), (None, None), (0, None)}
    for c in big:
        p = plans[c.id]
        assert p["per_slab"] == 32 and not p["capped"]
        assert (p["items"], p["min_items"]) == ((48, 1) if c.gth == 16 else (96, 3)), c.id
    assert plans[next(c.id for c in WGRAD if (c.n, c.H, c.W) == (48, 17, 9))]["TH"] == 16
    capped = [c for c in WGRAD if plans[c.id]["capped"] and (c.n, c.H, c.W, c.C) == (2, 9, 33, 64)]
    assert capped and plans[capped[0].id]["per_slab"] == 8 and plans[capped[0].id]["max_items"] == 1


@pytest.mark.parametrize("case", [c for c in R.CASES if c.regime != "gaussian"], ids=lambda c: c.id)
def test_a_bar_of_zero_is_justified_by_the_reference_alone(case):
    d, ref = R.prepared(case)
    assert not R.exactness_violations(case, d, ref)
    for t in d.values():                                  # every operand is exact in the type the kernel reads it in
        if t is not None:
            assert torch.equal(t.to(torch.float32).to(R.F64), t)
    for name in ("x", "dy", "add"):
        if d.get(name) is not None:
            assert torch.equal(R._rb(d[name]), d[name]), name
    assert torch.equal(R._rb(d["w49"]), d["w49"]) if case.op == "conv" else True      # exact as bf16 taps too


def _front(case, d, ref):
    """Image 0 alone of a large conv case (data and reference)."""
    cut = lambda t: t[0:1] if t is not None and t.dim() == 4 else t
    return case._replace(n=1), {k: cut(v) for k, v in d.items()}, {k: cut(v) for k, v in ref.items()}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_the_emulation_is_inside_every_bar_and_every_mutation_leaves_it(case):
    d, ref = R.prepared(case)
    if case.op == "conv":
        c1, d1, r1 = _front(case, d, ref) if case.n * case.H * case.W * case.C > BIG else (case, d, ref)
        worst, _ = R.check_conv(c1, r1, R.emulate_conv(c1, d1))
        assert worst <= 1.0, worst
        for m in R.CONV_MUTATIONS:
            if R.mutation_applies(case, m):
                got, sel = R.emulate_conv(case, d, m)
                assert R.check_conv(case, ref, got, sel)[0] > 1.0, m
    else:
        dw, db = R.emulate_wgrad(case, d)
        res = R.check_wgrad(case, ref, dw, db)
        assert all(v <= 1.0 for v in res.values()), res
        for m in R.WGRAD_MUTATIONS:
            if R.mutation_applies(case, m):
                dw, db, sel = R.emulate_wgrad(case, d, m)
                res = R.check_wgrad(case, ref, dw, db, sel)
                assert res["dbias" if m == "dbias_oob" else "dw"] > 1.0, (m, res)


def test_the_measured_weight_gradient_constant_meets_its_conditions():
    """K_DW is measured on the GPU; what it may not be is decided here: no larger than the term count of the smallest gaussian case
    (a bar that wide would pass a sum with every term rounded away), and one dropped pixel leaves the bar there."""
    g = [c for c in WGRAD if c.regime == "gaussian"]
    small = min(g, key=lambda c: c.n * c.H * c.W)
    assert (small.n, small.H, small.W) == (2, 3, 5) and R.K_DW <= small.n * small.H * small.W
    d, ref = R.prepared(small)
    dw, db, sel = R.emulate_wgrad(small, d, "pixel_dropped")
    assert R.check_wgrad(small, ref, dw, db, sel)["dw"] > 1.0
    assert R.K_DW == 2.0 ** round(torch.log2(torch.tensor(R.K_DW)).item())


def test_reference_gradients_are_the_autograd_gradients():
    """conv64 with flipped taps and wgrad64 against torch autograd of F.conv2d in float64."""
    case = next(c for c in CONV if c.regime == "gaussian" and (c.n, c.H, c.W) == (3, 37, 50) and not c.mfma and not c.flip)
    d, ref = R.prepared(case)
    x = d["x"].permute(0, 3, 1, 2).clone().requires_grad_(True)
    w = d["w49"].t().reshape(case.C, 1, 7, 7).clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(x, w, d["bias"], padding=3, groups=case.C)
    assert torch.allclose(y.detach().permute(0, 2, 3, 1), ref["pre"], rtol=1e-12, atol=1e-13)
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(y.shape, generator=g, dtype=R.F64)
    y.backward(dy)
    dyl = dy.permute(0, 2, 3, 1).contiguous()
    assert torch.allclose(R.conv64(dyl, d["w49"], None, None, flip=True), x.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-13)
    dw, db = R.wgrad64(d["x"], dyl)
    assert torch.allclose(dw, w.grad.reshape(case.C, 49).t(), rtol=1e-12, atol=1e-11)
    assert torch.allclose(db, dyl.sum((0, 1, 2)), rtol=1e-12, atol=1e-11)
