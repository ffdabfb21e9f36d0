"""tests/softmax_ref.py checked on the CPU: the float64 references against independent statements (torch's float64 autograd of
cross_entropy on s X Y^T and its transpose; the oracle's clip_loss and averaged_medical_clip_loss), the exactness preconditions on
the reference alone, the fp32 emulation of the kernels inside every bar (bit for bit in the exact regimes) and every mutation of it
outside them wherever the case contains the mutated feature - at the committed K_EXP / K_LOG."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import softmax_ref as R

TOL = 1e-12


def _close(got, want):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert float((got - want).abs().max()) <= TOL * max(1.0, float(want.abs().max())), float((got - want).abs().max())


def _val(case):
    return {k: v for k, (v, _) in R.reference(case).items()}


def test_rows_and_their_gradients_agree_with_cross_entropy_autograd():
    """CE(s X Y^T, labels, sum) * coef in float64: lse / pos, the ROW rule's dX and dscale, and the COL rule as the gradient of the
    same loss with respect to Y (the transposed problem: rows Y, columns X, key r = r)."""
    n, N, D = 37, 29, 64
    X, Y = R.gaussian_case(n, N, D, seed=5)
    s, coef = R.f32(14.2857), 0.125
    lab = (7 * torch.arange(n) + 3) % N
    Xa, Ya = X.double().requires_grad_(True), Y.double().requires_grad_(True)
    sa = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    z = sa * (Xa @ Ya.t())
    loss = coef * F.cross_entropy(z, lab, reduction="sum")
    loss.backward()
    fwd = _val(R._case("fwd_label", X, Y, s, row_label=lab))
    _close(fwd["lse"], torch.logsumexp(z.detach(), 1))
    _close(fwd["pos"], z.detach()[torch.arange(n), lab])
    _close(coef * (fwd["lse"] - fwd["pos"]).sum(), loss.detach())
    row = _val(R._case("row", X, Y, s, lse_row=fwd["lse"], row_label=lab, coef=coef, dscale0=0.0))
    _close(row["dX"], Xa.grad)
    _close(row["dscale"], sa.grad)
    col = _val(R._case("col", Y, X, s, lse_col=fwd["lse"], col_label=lab, key_off=0, coef=coef))
    _close(col["dX"], Ya.grad)
    dense = _val(R._case("dense", X, Y, s, Ga=torch.ones(n, N), lda=N, Gb=2 * torch.ones(N, n), ldb=n, dscale0=0.0))
    _close(dense["dX"], s * 3 * Y.double().sum(0)[None, :].expand(n, D))
    _close(dense["dscale"], 3 * (X.double() @ Y.double().t()).sum())


def test_diag_forward_and_fused_rule_agree_with_the_oracle_clip_loss():
    from oracle import clip_oracle as O
    N, D = 64, 32
    img, txt = R.gaussian_case(N, N, D, seed=6)
    s = R.f32(14.2857)
    a, t = img.double().requires_grad_(True), txt.double().requires_grad_(True)
    sa = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    loss, _ = O.clip_loss(sa * a @ t.t(), sa * t @ a.t())
    loss.backward()
    coef = 1.0 / (2 * N)
    fi, ft = _val(R._case("fwd_diag", img, txt, s)), _val(R._case("fwd_diag", txt, img, s))
    _close(coef * ((fi["lse"] - fi["pos"]).sum() + (ft["lse"] - ft["pos"]).sum()), loss.detach())
    half = N // 2
    for r in range(2):                                  # two ranks' rows: diag_off
        sl = slice(r * half, (r + 1) * half)
        gi = _val(R._case("fused", img[sl], txt, s, diag_off=r * half, lse_row=fi["lse"][sl], lse_col=ft["lse"], coef=coef, dscale0=0.0))
        gt = _val(R._case("fused", txt[sl], img, s, diag_off=r * half, lse_row=ft["lse"][sl], lse_col=fi["lse"], coef=coef, dscale0=0.0))
        _close(gi["dX"], a.grad[sl])
        _close(gt["dX"], t.grad[sl])
        fwd = _val(R._case("fwd_diag", img[sl], txt, s, diag_off=r * half))
        _close(fwd["lse"], fi["lse"][sl])
        _close(fwd["pos"], fi["pos"][sl])
    whole = _val(R._case("fused", img, txt, s, lse_row=fi["lse"], lse_col=ft["lse"], coef=coef, dscale0=0.0))
    _close(whole["dscale"], sa.grad)


def test_labelled_rules_agree_with_the_oracle_averaged_loss_at_k_below_n():
    """oracle.averaged_medical_clip_loss (float64 autograd) against the four launches of head.FusedAveragedLoss.backward restated
    with the references: ROW + COL for the image rows, ROW + COL (keyed, with counts, on the centroid rows) for the text rows."""
    from oracle import clip_oracle as O
    from tests.test_averaged_fused_cpu import THRESHOLD, assert_threshold_margin, clustered_inputs
    N, D = 64, 32
    img, txt = clustered_inputs(N, D, 7, seed=2)
    assert_threshold_margin(txt)
    ie, te = F.normalize(img.double(), dim=1).requires_grad_(True), F.normalize(txt.double(), dim=1).requires_grad_(True)
    s = R.f32(14.2857)
    sa = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    loss, labels = O.averaged_medical_clip_loss(ie, te, sa, sa * ie @ te.t(), sa * te @ ie.t(), THRESHOLD)
    loss.backward()
    k = int(labels.max()) + 1
    assert k < N
    I, Tx = ie.detach(), te.detach()
    cent = R.cluster_centroids(Tx, labels, k)
    counts = torch.bincount(labels, minlength=k).to(torch.int32)
    coef = 1.0 / (2 * N)
    fi, ft = _val(R._case("fwd_label", I, cent, s, row_label=labels)), _val(R._case("fwd_label", Tx, I, s, row_label=labels))
    _close(coef * ((fi["lse"] - fi["pos"]).sum() + (ft["lse"] - ft["pos"]).sum()), loss.detach())
    di = _val(R._case("row", I, cent, s, lse_row=fi["lse"], row_label=labels, coef=coef, dscale0=0.0))
    di2 = _val(R._case("col", I, Tx, s, lse_col=ft["lse"], col_label=labels, key_off=0, coef=coef, accumulate=1, dX0=di["dX"]))
    _close(di2["dX"], ie.grad)
    dt = _val(R._case("row", Tx, I, s, lse_row=ft["lse"], row_label=labels, coef=coef, dscale0=float(di["dscale"])))
    dt2 = _val(R._case("col", cent[labels], I, s, lse_col=fi["lse"], col_label=labels, row_key=labels, counts=counts, coef=coef, accumulate=1,
                       dX0=dt["dX"]))
    _close(dt2["dX"], te.grad)
    _close(dt["dscale"], sa.grad)


def test_small_kernel_references_agree_with_autograd():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 96, generator=g)
    xa = x.double().requires_grad_(True)
    dy = torch.randn(5, 96, generator=g)
    y = xa / xa.norm(dim=1, keepdim=True)
    y.backward(dy.double())
    f = R.l2norm_fwd(x)
    _close(f["y"][0], y.detach())
    _close(R.l2norm_bwd(y.detach(), f["norm"][0], dy)["dx"][0], xa.grad)
    z = torch.randn(5, 65, generator=g) * 4
    lab = torch.tensor([0, 64, 3, 3, 17])
    for labels in (lab, None):
        za = z.double().requires_grad_(True)
        loss = 0.5 * F.cross_entropy(za, torch.arange(5) if labels is None else labels, reduction="sum")
        (0.25 * loss).backward()
        f = R.ce_rows_fwd(z, labels, 0.5, 0.0)
        _close(f["loss"][0], loss.detach())
        _close(R.ce_rows_bwd(z, labels, f["lse"][0], 0.25, 0.5)["dlogits"][0], za.grad)
    lse, pos = torch.randn(257, generator=g) + 5, torch.randn(257, generator=g)
    _close(R.loss_reduce(lse, pos, None, None, 0.25, 0.5)["loss"][0], 0.5 + 0.25 * (lse.double() - pos.double()).sum())
    _close(R.loss_reduce(lse, pos, pos, lse, 0.25, 0.5)["loss"][0], 0.5)
    labels = torch.tensor([0, 1, 1, 2, 0, 1, 3])
    za = torch.randn(4, 7, generator=g).double().requires_grad_(True)
    from oracle import clip_oracle as O
    want = O.average_logits(za, labels.tolist())
    dout = torch.randn(4, 4, generator=g)
    want.backward(dout.double())
    f, counts = R.cluster_mean_cols_fwd(za.detach(), labels, 4)
    _close(f["out"][0], want.detach())
    assert counts.tolist() == [2, 3, 1, 1]
    _close(R.cluster_mean_cols_bwd(dout, labels, counts)["dlogits"][0], za.grad)
    T = torch.randn(7, 32, generator=g)
    cent = R.cluster_centroids(T, labels, 5)
    _close(cent[1], T.double()[[1, 2, 5]].mean(0))
    assert bool((cent[4] == 0).all())


@functools.lru_cache(maxsize=None)
def _gauss(shape, scale):
    cases = R.gaussian_cases(shape, scale)
    return {k: (c, R.reference(c)) for k, c in cases.items()}


@pytest.mark.parametrize("shape", R.SHAPES)
def test_emulation_is_inside_every_bar(shape):
    for scale in R.SCALES + (1.0,):
        for name, (c, ref) in _gauss(shape, scale).items():
            if scale == 1.0 and c.op != "dense":
                continue
            q = R.ratios(ref, R.emulate(c))
            assert max(q.values()) <= 1.0, (scale, name, q)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_exact_regime_preconditions_and_emulation(shape):
    for name, c in R.exact_cases(shape).items():
        ref = R.reference(c)
        assert R.exactness_violations(c, ref) == [], name
        assert R.exact_mismatches(c, ref, R.emulate(c)) == [], name
        q = R.ratios(ref, R.emulate(c))                       # the bars hold in the exact regime too
        assert max(q.values()) <= 1.0, (name, q)


def test_exactness_violations_reject_vacuous_and_inexact_cases():
    shape = (33, 33, 64, 0)
    c = R.onehot_case(shape, "row")
    c.X = c.Y.clone()[:33]
    c.row_label = torch.arange(33)
    c.Y = torch.eye(33, 64)
    c.X = torch.eye(33, 64)                              # each row's label column is its only matching column: every g is 0
    assert any("vacuous" in b for b in R.exactness_violations(c, R.reference(c)))
    c = R.onehot_case(shape, "fused", gout=0.3)
    assert any("power of two" in b for b in R.exactness_violations(c, R.reference(c)))
    c = R.onehot_case(shape, "fwd_diag")
    c.Y = torch.zeros_like(c.Y)
    c.Y[:, 0] = 1.0                                       # a row matches every column or none
    assert any("vacuous" in b for b in R.exactness_violations(c, R.reference(c)))
    c = R.integer_case(shape, "dense")
    c.Gb = c.Ga[:, :33].t().contiguous().clone()          # g symmetric: a transposed read cannot show
    c.Gb, c.Ga = c.Gb * 0, c.Ga * 0
    assert any("vacuous" in b for b in R.exactness_violations(c, R.reference(c)))
    c = R.integer_case(shape, "dense")
    c.X = c.X + 0.5
    assert any("not integer" in b for b in R.exactness_violations(c, R.reference(c)))
    c = R.gaussian_cases(shape, 14.2857)["fused"]
    assert R.exactness_violations(c, R.reference(c)) == ["not an exact case"]


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_leaves_a_bar_or_breaks_an_equality(mut):
    """At the committed K_EXP / K_LOG.  Gaussian regime: EVERY case that contains the mutated feature must leave a bar.  Exact regimes:
    the cases that contain it are counted; those whose data cannot show it (every lse input is 256, so lse_col_by_row reads the same
    number; one-hot maxima never grow by less than 256) are the Gaussian regime's business."""
    seen = broken_exact = 0
    for shape in R.SHAPES:
        for scale in R.SCALES:
            for name, (c, ref) in _gauss(shape, scale).items():
                if not R.mutation_applies(c, mut):
                    continue
                q = R.ratios(ref, R.emulate(c, mut))
                assert max(q.values()) > 1.0, (mut, shape, scale, name, q)
                seen += 1
        for name, c in R.exact_cases(shape).items():
            if R.mutation_applies(c, mut) and R.exact_mismatches(c, R.reference(c), R.emulate(c, mut)):
                broken_exact += 1
    assert seen >= 1, "no Gaussian case contains the feature"
    if mut not in ("lse_col_by_row", "no_rescale"):
        assert broken_exact >= 1, "no exact case shows the mutation"


def test_no_rescale_is_visible_at_the_shape_with_a_fifth_column_tile():
    shape = (32, R.COLS_PER_PASS + 1, 512, 0)
    for scale in R.SCALES:
        assert R.mutation_applies(_gauss(shape, scale)["fwd"][0], "no_rescale"), scale


def test_shapes_reach_every_instantiation_and_both_store_paths():
    assert {R.ndt_of(s[2]) for s in R.SHAPES} == {1, 2, 4, 8}
    assert {s[2] // 32 % 4 for s in R.SHAPES if R.ndt_of(s[2]) in (1, 2)} >= {1, 3}       # waves without a d tile: D = 96, 160
    assert any(s[1] % 4 and s[1] > 4 for s in R.SHAPES) and any(s[1] < 32 and s[1] % 4 for s in R.SHAPES)
    assert any(s[3] for s in R.SHAPES) and any(s[1] == R.COLS_PER_PASS + 1 for s in R.SHAPES) and any(s[0] > s[1] for s in R.SHAPES)
    assert R.kernel_note("fused", 160) == "rows_bwd_kernel<ClipFusedPair, 2>" and R.kernel_note("fwd_label") == "rows_lse_fwd_kernel<RowLabel, false>"
    assert math.ceil(129 / 32) == 5
