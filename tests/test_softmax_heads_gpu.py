"""The softmax contrastive heads on the MI355X: every entry point of csrc/clip_head.hip and csrc/averaged_head.hip on the tile skeleton
csrc/clip_tile.h, and the small kernels around it, through `_hip.call` on the test's own buffers, against the float64 references and
the derived bars of tests/softmax_ref.py.

Every call writes into buffers pre-filled with NaN bits (accumulated scalars with 0.5, an accumulated dX with a known matrix) and
followed by 32 sentinel entries or rows; the pad columns of a pitched output hold sentinels too.  No owned element may keep a NaN and
no sentinel may change.  Every launch of the skeleton runs with the kernel notes on and must name the instantiation
softmax_ref.kernel_note expects, so the four NDT instantiations of the four pair rules, both label sources and both WRITE_LOGITS
flavours are proved reached (test_planned_kernels_are_the_ones_launched spells the table out).

Gaussian regime: softmax_ref.SHAPES x SCALES (the dense rule at s = 1 as well), every case of softmax_ref.gaussian_cases inside its
bars; the worst ratios go through conftest.measured (committed copy: profiles/softmax_measured_tolerances.jsonl).
Exact regimes (torch.equal): softmax_ref.exact_cases, preconditions asserted on the reference alone."""
import functools
import math

import pytest
import torch

from tests import softmax_ref as R
from tests.conftest import measured

pytestmark = pytest.mark.gpu
TAIL = 32
SENTINEL = 12345.0
NAN_BITS = 0x7FC00ABC
F0 = 0.5


def _out(dev, rows, cols=None, fill=None, pitch=None):
    """rows (+ TAIL sentinel rows) of NaN bits, or of `fill`; with a pitch, the columns from `cols` on hold sentinels."""
    shape = (rows + TAIL,) if cols is None else (rows + TAIL, pitch or cols)
    t = torch.full(shape, SENTINEL, device=dev, dtype=torch.float32)
    own = t[:rows] if cols is None else t[:rows, :cols]
    if fill is None:
        own.copy_(torch.full((1,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32).expand_as(own))
    else:
        own.copy_(torch.as_tensor(fill, dtype=torch.float32).to(dev).expand_as(own))
    return t


def _take(t, rows, cols=None, nan_ok=None):
    assert bool((t[rows:] == SENTINEL).all()), "a sentinel after the output changed"
    if cols is not None:
        assert bool((t[:rows, cols:] == SENTINEL).all()), "a sentinel in the pad columns changed"
    out = (t[:rows] if cols is None else t[:rows, :cols]).cpu()
    bad = torch.isnan(out)
    if nan_ok is not None:
        bad[nan_ok] = False
    assert not bool(bad.any()), "an owned element kept its NaN fill (or the kernel produced one)"
    return out


def _dev(dev, t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).to(dev).contiguous()


def _scalar(dev, v):
    return None if v is None else torch.tensor([v], device=dev, dtype=torch.float32)


def _launch(dev, c):
    """One launch of the case's entry point on fresh buffers -> name -> CPU tensor, as softmax_ref.reference names them."""
    from mmgclip import _hip
    from mmgclip._hip import call, ptr, stream
    lib = _hip.load()
    n, N, D = c.n, c.N, c.D
    X, Y, s = _dev(dev, c.X.float()), _dev(dev, c.Y.float()), _scalar(dev, c.s)
    keep, outs = [X, Y, s], {}
    if c.op in ("fwd_diag", "fwd_label"):
        lse, pos = _out(dev, n), _out(dev, n)
        logits = None if c.ldl is None else _out(dev, n, N, pitch=c.ldl)
        if c.op == "fwd_diag":
            fn = lambda: call("mmg_clip_rows_fwd", ptr(X), ptr(Y), ptr(s), n, N, D, c.diag_off, ptr(lse), ptr(pos), ptr(logits), c.ldl or 0, stream())
        else:
            lab = _dev(dev, c.row_label, torch.int64)
            keep.append(lab)
            fn = lambda: call("mmg_clip_labelled_rows_fwd", ptr(X), ptr(Y), ptr(s), ptr(lab), n, N, D, ptr(lse), ptr(pos), stream())
        take = lambda: {"lse": _take(lse, n), "pos": _take(pos, n), **({} if logits is None else {"logits": _take(logits, n, N)})}
    else:
        dX = _out(dev, n, D, fill=c.dX0 if c.accumulate else None)
        ds = None if (c.dscale0 is None or c.op == "col") else _out(dev, 1, fill=c.dscale0)
        gout = _scalar(dev, c.gout)
        lr, lc = _dev(dev, c.lse_row, torch.float32), _dev(dev, c.lse_col, torch.float32)
        if c.op == "fused":
            fn = lambda: call("mmg_clip_rows_bwd_fused", ptr(X), ptr(Y), ptr(s), ptr(lr), ptr(lc), ptr(gout), c.coef, n, N, D, c.diag_off,
                              ptr(dX), ptr(ds), stream())
        elif c.op == "dense":
            Ga, Gb = _dev(dev, c.Ga), _dev(dev, c.Gb)
            keep += [Ga, Gb]
            fn = lambda: call("mmg_clip_rows_bwd_dense", ptr(X), ptr(Y), ptr(s), ptr(Ga), c.lda or 0, ptr(Gb), c.ldb or 0, n, N, D, ptr(dX),
                              ptr(ds), stream())
        elif c.op == "row":
            lab = _dev(dev, c.row_label, torch.int64)
            keep.append(lab)
            fn = lambda: call("mmg_clip_labelled_rows_bwd_row", ptr(X), ptr(Y), ptr(s), ptr(lr), ptr(lab), ptr(gout), c.coef, n, N, D,
                              c.accumulate, ptr(dX), ptr(ds), stream())
        else:
            lab, key, cnt = _dev(dev, c.col_label, torch.int64), _dev(dev, c.row_key, torch.int64), _dev(dev, c.counts, torch.int32)
            keep += [lab, key, cnt]
            fn = lambda: call("mmg_clip_labelled_rows_bwd_col", ptr(X), ptr(Y), ptr(s), ptr(lc), ptr(lab), ptr(key), c.key_off, ptr(cnt),
                              0 if cnt is None else cnt.shape[0], ptr(gout), c.coef, n, N, D, c.accumulate, ptr(dX), stream())
        take = lambda: {"dX": _take(dX, n), **({} if ds is None else {"dscale": _take(ds, 1)[0]})}
    torch.cuda.synchronize()
    lib.mmg_set_kernel_notes(1)
    try:
        fn()
        note = lib.mmg_last_kernel().decode()
    finally:
        lib.mmg_set_kernel_notes(0)
    torch.cuda.synchronize()
    assert note == R.kernel_note(c.op, D, c.ldl is not None), note
    outs = take()
    outs["note"] = note
    return outs


@functools.lru_cache(maxsize=None)
def _gauss(shape, scale):
    """Cases and float64 references of one shape and scale, computed once and shared (read-only)."""
    cases = R.dense_scale_cases(shape) if scale == 1.0 else R.gaussian_cases(shape, scale)
    return {k: (c, R.reference(c)) for k, c in cases.items()}


@pytest.mark.parametrize("shape", R.SHAPES)
def test_gaussian_regime_inside_the_bars(dev, shape):
    worst = {}
    for scale in R.SCALES + (1.0,):
        for name, (c, ref) in _gauss(shape, scale).items():
            q = R.ratios(ref, _launch(dev, c))
            print(shape, scale, name, q)
            for out, v in q.items():
                key = f"{c.op}.{out}"
                worst[key] = max(worst.get(key, 0.0), v)
    measured("softmax_gaussian", shape=str(shape), k_exp=R.K_EXP, k_log=R.K_LOG, **worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("shape", R.SHAPES)
def test_exact_regimes_are_bit_exact(dev, shape):
    for name, c in R.exact_cases(shape).items():
        ref = R.reference(c)
        assert R.exactness_violations(c, ref) == [], name
        assert R.exact_mismatches(c, ref, _launch(dev, c)) == [], name


def test_planned_kernels_are_the_ones_launched(dev):
    """One case per NDT in {1, 2, 4, 8} and pair rule, and both label sources with and without logits: mmg_last_kernel() names the
    instantiation the shape should take (D = 96 -> 1, 160 -> 2, 512 -> 4, 1024 -> 8)."""
    seen = set()
    for shape, ndt in (((33, 33, 96, 0), 1), ((34, 35, 160, 0), 2), ((32, R.COLS_PER_PASS + 1, 512, 0), 4), ((65, 65, 1024, 0), 8)):
        cases = R.exact_cases(shape)
        for name, pair in (("hot_fused", "ClipFusedPair"), ("int_dense_ab", "ClipDensePair"), ("hot_row", "LabelledRowPair"),
                           ("hot_col_key", "LabelledColPair")):
            note = _launch(dev, cases[name])["note"]
            assert note == f"rows_bwd_kernel<{pair}, {ndt}>", (shape, name, note)
            seen.add(note)
        for name, want in (("hot_fwd", "rows_lse_fwd_kernel<DiagLabel, false>"), ("int_logits_ld4", "rows_lse_fwd_kernel<DiagLabel, true>"),
                           ("hot_fwd_label", "rows_lse_fwd_kernel<RowLabel, false>")):
            note = _launch(dev, cases[name])["note"]
            assert note == want, (shape, name, note)
            seen.add(note)
    assert len(seen) == 16 + 3


def test_two_simulated_ranks_equal_one_launch_and_the_unsharded_reference(dev):
    """(64, 128, 512) twice: rank r holds rows 64 r .. 64 r + 63 of the 128.  A row's results do not depend on the rows around it, so
    lse, pos and dX are those of one launch at n_loc = 128 bit for bit; dscale is the sum over the ranks, inside its bar."""
    N, D, nl = 128, 512, 64
    X, Y = R.gaussian_case(N, N, D, seed=11)
    s, coef = R.f32(14.2857), R.f32(1.0 / (2 * N))
    z = s * (X.double() @ Y.double().t())
    lse_row, lse_col = torch.logsumexp(z, 1).float(), torch.logsumexp(z, 0).float()
    rl, cl = R.row_labels(N, N), R.hand_labels(N)

    def case(op, sl, off, ranks=1):
        kw = dict(fwd_diag=dict(diag_off=off),
                  fused=dict(diag_off=off, lse_row=lse_row[sl], lse_col=lse_col, coef=coef, gout=0.25, dscale0=F0 * ranks, ranks=ranks),
                  row=dict(lse_row=lse_row[sl], row_label=rl[sl], coef=coef, gout=0.25, dscale0=F0 * ranks, ranks=ranks),
                  col=dict(lse_col=lse_col, col_label=cl, key_off=off, coef=coef, gout=0.25))[op]
        return R._case(op, X[sl], Y, s, **kw)
    worst = {}
    for op in ("fwd_diag", "fused", "row", "col"):
        parts = []
        for r in range(2):
            parts.append(_launch(dev, case(op, slice(r * nl, (r + 1) * nl), r * nl)))
        one = _launch(dev, case(op, slice(0, N), 0))
        got = {}
        for name in one:
            if name in ("note", "dscale"):
                continue
            got[name] = torch.cat([p[name] for p in parts])
            assert torch.equal(got[name], one[name]), (op, name)
        if "dscale" in one:
            got["dscale"] = parts[0]["dscale"] + parts[1]["dscale"]
        q = R.ratios(R.reference(case(op, slice(0, N), 0, ranks=2)), got)
        print(op, q)
        worst.update({f"{op}.{k}": v for k, v in q.items()})
    measured("softmax_two_ranks", k_exp=R.K_EXP, k_log=R.K_LOG, **worst)
    assert max(worst.values()) <= 1.0, worst


def test_rows_are_bit_identical_over_three_runs(dev):
    cases = _gauss((32, R.COLS_PER_PASS + 1, 512, 0), R.SCALES[0])
    for name in ("fwd_logits_ld4", "fused_gout", "row_acc", "col_key"):
        runs = [_launch(dev, cases[name][0]) for _ in range(3)]
        for k in runs[0]:
            if k not in ("note", "dscale"):
                assert all(torch.equal(r[k], runs[0][k]) for r in runs[1:]), (name, k)


# ---------------------------------------------------------------------------------------------------------------------------------
# the small kernels around the skeleton
# ---------------------------------------------------------------------------------------------------------------------------------
def _go(name, *args):
    from mmgclip._hip import call, stream
    call(name, *args, stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", [32, 96, 1024])
@pytest.mark.parametrize("rows", [1, 5, 37])
def test_l2norm_forward_and_backward(dev, rows, D):
    """A zero row gives norm 0 and y = 0 / 0 = NaN, as the reference does (no epsilon); it is asserted on the row appended for it and
    kept out of the other rows' comparison."""
    from mmgclip._hip import ptr
    g = torch.Generator().manual_seed(100 * rows + D)
    x = torch.cat([torch.randn(rows, D, generator=g) * 3, torch.zeros(1, D)])
    n = rows + 1
    xd = _dev(dev, x)
    y, norm = _out(dev, n, D), _out(dev, n)
    _go("mmg_l2norm_fwd", ptr(xd), ptr(y), ptr(norm), n, D)
    zero = torch.zeros(n, dtype=torch.bool)
    zero[rows] = True
    yh, nh = _take(y, n, nan_ok=zero), _take(norm, n)
    assert bool(torch.isnan(yh[rows]).all()) and float(nh[rows]) == 0.0
    ref = R.l2norm_fwd(x[:rows])
    q = R.ratios(ref, {"y": yh[:rows], "norm": nh[:rows]})
    dy = torch.randn(rows, D, generator=g)
    dyd, yd, nd = _dev(dev, dy), _dev(dev, yh[:rows]), _dev(dev, nh[:rows])
    dx = _out(dev, rows, D)
    _go("mmg_l2norm_bwd", ptr(yd), ptr(nd), ptr(dyd), ptr(dx), rows, D)
    q.update(R.ratios(R.l2norm_bwd(yh[:rows], nh[:rows], dy), {"dx": _take(dx, rows)}))
    print(rows, D, q)
    measured("softmax_l2norm", rows=rows, D=D, **q)
    assert max(q.values()) <= 1.0, q


@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("C", [1, 5, 65, 200])
def test_ce_rows_forward_and_backward(dev, C, with_labels):
    """ld > C with large pad columns (a leak into a row's lse would show), weight = 0.5, labels in range or NULL (then rows <= C)."""
    from mmgclip._hip import ptr
    g = torch.Generator().manual_seed(C)
    rows = 37 if with_labels else min(C, 37)
    ld, ldd = C + 3, C + 5
    z = torch.full((rows, ld), 1.0e4)
    z[:, :C] = torch.randn(rows, C, generator=g) * 6
    labels = torch.randint(0, C, (rows,), generator=g) if with_labels else None
    zd, ld_ = _dev(dev, z), _dev(dev, labels, torch.int64)
    lse, loss = _out(dev, rows), _out(dev, 1, fill=F0)
    _go("mmg_ce_rows_fwd", ptr(zd), ld, ptr(ld_), rows, C, 0.5, ptr(lse), ptr(loss))
    lse_h = _take(lse, rows)
    q = R.ratios(R.ce_rows_fwd(z[:, :C], labels, 0.5, F0), {"lse": lse_h, "loss": _take(loss, 1)[0]})
    for gout in (None, 0.25):
        d = _out(dev, rows, C, pitch=ldd)
        gd, lsed = _scalar(dev, gout), _dev(dev, lse_h)
        _go("mmg_ce_rows_bwd", ptr(zd), ld, ptr(ld_), ptr(lsed), ptr(gd), 0.5, rows, C, ptr(d), ldd)
        qb = R.ratios(R.ce_rows_bwd(z[:, :C], labels, lse_h, gout, 0.5), {"dlogits": _take(d, rows, C)})
        q["dlogits"] = max(q.get("dlogits", 0.0), qb["dlogits"])
    print(C, with_labels, q)
    measured("softmax_ce_rows", C=C, labels=int(with_labels), k_exp=R.K_EXP, k_log=R.K_LOG, **q)
    assert max(q.values()) <= 1.0, q


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_clip_loss_reduce_one_and_two_sided(dev, n):
    from mmgclip._hip import ptr
    g = torch.Generator().manual_seed(n)
    la, pa, lb, pb = (torch.randn(n, generator=g) * 3 + k for k in (5.0, 0.0, 4.0, 1.0))
    d = [_dev(dev, t) for t in (la, pa, lb, pb)]
    q = {}
    for two in (False, True):
        loss = _out(dev, 1, fill=F0)
        _go("mmg_clip_loss_reduce", ptr(d[0]), ptr(d[1]), ptr(d[2]) if two else None, ptr(d[3]) if two else None, n, 0.25, ptr(loss))
        ref = R.loss_reduce(la, pa, lb if two else None, pb if two else None, 0.25, F0)
        q["two_sided" if two else "one_sided"] = R.ratios(ref, {"loss": _take(loss, 1)[0]})["loss"]
    print(n, q)
    measured("softmax_loss_reduce", n=n, **q)
    assert max(q.values()) <= 1.0, q


@pytest.mark.parametrize("k", [1, 3, 300])
def test_cluster_mean_cols_forward_and_backward(dev, k):
    """N = 300 columns: more than the 256 threads of a row's workgroup, so with k = 3 (labels j % 3) and k = 1 a cluster's members are
    added by different passes of the stride; k = N is every column its own cluster.  Strided ld / ldo.  The forward's LDS float
    atomics have no fixed order: the bar ((c - 1) u sum |.|) holds for any."""
    from mmgclip._hip import ptr
    n, N = 3, 300
    g = torch.Generator().manual_seed(k)
    labels = torch.arange(N) % k
    ld, ldo = N + 3, k + 2
    z = torch.full((n, ld), 1.0e4)
    z[:, :N] = torch.randn(n, N, generator=g) * 5
    ref, counts = R.cluster_mean_cols_fwd(z[:, :N], labels, k)
    zd, lab, cnt = _dev(dev, z), _dev(dev, labels, torch.int64), _dev(dev, counts, torch.int32)
    out = _out(dev, n, k, pitch=ldo)
    _go("mmg_cluster_mean_cols_fwd", ptr(zd), ld, n, N, ptr(lab), ptr(cnt), k, ptr(out), ldo)
    q = R.ratios(ref, {"out": _take(out, n, k)})
    dout = torch.full((n, ldo), 1.0e4)
    dout[:, :k] = torch.randn(n, k, generator=g)
    dd = _dev(dev, dout)
    dl = _out(dev, n, N, pitch=ld)
    _go("mmg_cluster_mean_cols_bwd", ptr(dd), ldo, n, N, ptr(lab), ptr(cnt), ptr(dl), ld)
    q.update(R.ratios(R.cluster_mean_cols_bwd(dout[:, :k], labels, counts), {"dlogits": _take(dl, n, N)}))
    print(k, q)
    measured("softmax_cluster_mean_cols", k=k, **q)
    assert max(q.values()) <= 1.0, q


def test_cluster_centroids_exact_empty_and_deterministic(dev):
    """Small-integer rows and member counts 1, 2, 4, 8, 0, 16, 64 (95 rows: more than one 64-label pass): every partial sum and every
    division is exact.  The empty cluster id gives a zero row.  Two runs give equal bits, on Gaussian rows as well, and the Gaussian
    centroids lie within c u sum |.| of the float64 means (ascending order: c - 1 additions and the division)."""
    from mmgclip._hip import ptr
    counts = [1, 2, 4, 8, 0, 16, 64]
    k, N, D = len(counts), sum(counts), 96
    g = torch.Generator().manual_seed(9)
    labels = torch.tensor([c for c, m in enumerate(counts) for _ in range(m)])[torch.randperm(N, generator=g)]
    assert torch.bincount(labels, minlength=k).tolist() == counts
    for T, exact in ((torch.randint(-3, 4, (N, D), generator=g).float(), True), (torch.randn(N, D, generator=g), False)):
        Td, lab = _dev(dev, T), _dev(dev, labels, torch.int64)
        runs = []
        for _ in range(2):
            out = _out(dev, k, D)
            _go("mmg_cluster_centroids", ptr(Td), ptr(lab), N, D, k, ptr(out))
            runs.append(_take(out, k))
        want = R.cluster_centroids(T, labels, k)
        assert torch.equal(runs[0], runs[1]) and bool((runs[0][4] == 0).all())
        if exact:
            assert torch.equal(runs[0], want.float())
        else:
            onehot = (labels[:, None] == torch.arange(k)[None, :]).double()
            bar = torch.tensor(counts).double()[:, None] * R.U * (onehot.t() @ T.double().abs()) / torch.tensor(counts).double().clamp(min=1)[:, None]
            assert R.ratio(runs[0], want, bar) <= 1.0


def _threshold_sim(n, ld, seed, thr):
    """[n, ld] similarities, none within 1e-2 of the threshold; the pad columns hold 1 (>= thr: a wrong pitch would show)."""
    g = torch.Generator().manual_seed(seed)
    sim = torch.full((n, ld), 1.0)
    v = torch.rand(n, n, generator=g) * 0.9
    v = torch.where((v - thr).abs() < 1e-2, v + 0.05, v)
    sim[:, :n] = v
    return sim


@pytest.mark.parametrize("n", [1, 33, 1025])
def test_greedy_threshold_labels(dev, n):
    """Against the oracle's first-fit double loop.  n = 1025 is more rows than threads.  Rows 0..2 hold a chain (0 ~ 1, 1 ~ 2, 0 !~ 2):
    2 must open its own cluster, so the order matters; a NaN similarity never joins a cluster; ld > n."""
    from mmgclip._hip import ptr
    from oracle import clip_oracle as O
    thr, ld = 0.65, n + 7
    sim = _threshold_sim(n, ld, n, thr)
    if n >= 33:
        sim[0, 1], sim[1, 2], sim[0, 2] = 0.9, 0.9, 0.1
        sim[0, 5] = sim[3, 7] = sim[0, n - 1] = float("nan")
    core = sim[:, :n].double()
    assert float((core[~torch.isnan(core)] - float(R.f32(thr))).abs().min()) > 1e-3
    want = O.assign_labels(sim[:, :n], thr)
    if n >= 33:
        assert want[1] == 0 and want[2] != 0 and want[5] != 0
    simd = _dev(dev, sim)
    labels = torch.full((n + TAIL,), -7, device=dev, dtype=torch.int64)
    counts = torch.full((n + TAIL,), -7, device=dev, dtype=torch.int32)
    kk = torch.full((1 + TAIL,), -7, device=dev, dtype=torch.int32)
    _go("mmg_greedy_threshold_labels", ptr(simd), ld, n, thr, ptr(labels), ptr(counts), ptr(kk))
    assert bool((labels[n:] == -7).all()) and bool((counts[n:] == -7).all()) and bool((kk[1:] == -7).all())
    assert labels[:n].cpu().tolist() == want
    k = max(want) + 1
    assert int(kk[0]) == k and counts[:n].cpu().tolist() == torch.bincount(torch.tensor(want), minlength=n).tolist()
