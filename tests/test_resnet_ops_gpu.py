"""The ResNet-50 tower kernels of csrc/resnet_ops.hip, each against a plain float64 reference computed on the CPU from the same
bf16-rounded inputs: im2col / col2im (pure gathers: bit-exact, and each other's adjoint), the 3x3/2 max pool (bit-exact), batch
norm forward (statistics, running buffers, the fused apply) and backward (the two reductions, dx, dres, the accumulated
parameter gradients).

Every assertion is one of three kinds: bit-exact; one bf16 ulp against the float64 result; or a bar computed in the test from
the float64 / float32 references alone, never from the kernel's output.

About "one bf16 ulp": a kernel that evaluates a sum or a difference in fp32 and rounds once cannot be within one bf16 ulp *of the
result* where the terms cancel (the result is then far smaller than the terms, and so is its ulp; behind a ReLU the float64
result may even be a tiny negative number where fp32 gives a tiny positive one).  So every such bar is
    |kernel - bf16(ref64)| <= ulp_bf16(ref) + A,
with A the rounding of the fp32 evaluation itself, a few 2^-24 of the sum of the |terms|, written out beside each use.  A is four
orders of magnitude below the bf16 ulp of a typical element, so it lets nothing through that a bf16 comparison could see; the
number of elements that need it is recorded with the other measured values."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import measured

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64
EPS = 1e-5
MOM = 0.1
MOM32 = float(np.float32(MOM))            # what the C ABI's `float momentum` holds
U32 = 2.0 ** -24                          # unit round-off of fp32
NAME = "test_resnet_ops_gpu."


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def _K():
    from mmgclip import kernels as K
    return K


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _bf16_ulp(v):
    """Spacing of bf16 numbers at |v| (float64 in, float64 out); the smallest normal's spacing below that."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))        # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), e - 8)


def _check_bf16(got, ref64, allowance):
    """got (bf16, CPU) against ref64: returns (worst |got - bf16(ref)| / (ulp + allowance), share bit-equal to bf16(ref),
    share of elements further than one plain ulp from bf16(ref), i.e. the ones that need the allowance)."""
    refb = ref64.to(BF)
    diff = (got.to(F64) - refb.to(F64)).abs()
    ulp = _bf16_ulp(refb.to(F64))
    worst = (diff / (ulp + allowance)).max().item()
    return worst, (_bits(got) == _bits(refb)).double().mean().item(), (diff > ulp).double().mean().item()


def _conv_out(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _im2col_ref(x4, k, s, p, Kp):
    """Index-loop im2col of x4 [n,H,W,C] (any dtype, moved as it is): column (kh*k + kw)*C + c, zeros elsewhere."""
    n, H, W, C = x4.shape
    Ho, Wo = _conv_out(H, W, k, s, p)
    xp = torch.zeros(n, H + 2 * p, W + 2 * p, C, dtype=x4.dtype)
    xp[:, p:p + H, p:p + W] = x4
    col = torch.zeros(n, Ho, Wo, Kp, dtype=x4.dtype)
    for kh in range(k):
        for kw in range(k):
            t = kh * k + kw
            col[..., t * C:(t + 1) * C] = xp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s]
    return col.view(n * Ho * Wo, Kp)


def _col2im_ref(d, n, H, W, C, k, s, p, absolute=False):
    """float64 fold (the adjoint of _im2col_ref) of d [n*Ho*Wo, Kp]; the K padding is never read.  absolute: fold |d|."""
    Ho, Wo = _conv_out(H, W, k, s, p)
    d4 = d.view(n, Ho, Wo, -1)
    dxp = torch.zeros(n, H + 2 * p, W + 2 * p, C, dtype=F64)
    for kh in range(k):
        for kw in range(k):
            t = kh * k + kw
            term = d4[..., t * C:(t + 1) * C].to(F64)
            dxp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s] += term.abs() if absolute else term
    return dxp[:, p:p + H, p:p + W].reshape(n * H * W, C)


@functools.lru_cache(maxsize=None)
def _stem_kp():
    """The K the tower's own packing gives conv1 (7*7*8 = 392 padded up): the K padding of the stem's column matrix is live."""
    from mmgclip.networks.resnet import ResNetTower
    kp = ResNetTower._w2d(torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), 8).shape[1]
    assert kp > 392 and kp % 8 == 0
    return kp


# (n, H, W, C, k, stride, pad, Kp or None = the stem's)
GEOMS = [
    (2, 18, 22, 8, 7, 2, 3, None),       # stem form, K padding live
    (2, 9, 7, 64, 3, 1, 1, 576),         # 3x3 stride 1
    (3, 8, 8, 64, 3, 2, 1, 576),         # 3x3 stride 2
    (2, 7, 9, 128, 3, 2, 1, 1152),       # 3x3 stride 2, odd H and W
    (2, 8, 6, 256, 1, 2, 0, 256),        # shortcut gather
    (2, 7, 5, 256, 1, 2, 0, 256),        # shortcut gather, odd sizes
    (2, 1, 96, 8, 7, 2, 3, None),        # 1 x L degenerate image
    (8, 96, 96, 64, 3, 1, 1, 576),       # rows * Kp / 8 > 16384 * 256: im2col's grid-stride loop runs more than once
]
BIG = GEOMS[-1]
# pixels * C / 8 > 16384 * 256: col2im's own grid-stride loop runs more than once (a 1x1 "fold" is a copy, so this one is cheap)
COL2IM_LOOP = (8, 96, 96, 512, 1, 1, 0, 512)


def _geom(g):
    n, H, W, C, k, s, p, Kp = g
    return n, H, W, C, k, s, p, (_stem_kp() if Kp is None else Kp)


def _gid(g):
    return "x".join(str(v) for v in g[:7])


def _small_ints(shape, seed):
    return torch.randint(-2, 3, shape, generator=_gen(seed), dtype=torch.int8).to(BF)


# ---- 1. im2col ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GEOMS, ids=_gid)
def test_im2col_is_the_exact_gather(dev, g):
    from mmgclip._hip import call, ptr, stream
    n, H, W, C, k, s, p, Kp = _geom(g)
    Ho, Wo = _conv_out(H, W, k, s, p)
    x = torch.randn(n * H * W, C, generator=_gen(1)).to(BF)
    ref = _im2col_ref(x.view(n, H, W, C), k, s, p, Kp)
    xd = x.to(dev)
    col = torch.full((n * Ho * Wo, Kp), float("nan"), device=dev, dtype=BF)       # every element must be written
    call("mmg_im2col_nhwc", ptr(xd), ptr(col), n, H, W, C, k, k, s, p, Kp, stream())
    got = col.cpu()
    assert torch.equal(_bits(got), _bits(ref))
    if Kp > k * k * C:
        assert (_bits(got[:, k * k * C:]) == 0).all()                             # K padding: exact (+0) zeros
    assert torch.equal(_bits(_K().im2col(xd, n, H, W, C, k, s, p, Kp).cpu()), _bits(ref))      # the wrapper the tower calls


# ---- 2. col2im ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GEOMS + [COL2IM_LOOP], ids=_gid)
def test_col2im_integer_sums_are_exact(dev, g):
    """Integers in [-2, 2]: every sum is at most 2 * 49 = 98 in magnitude, exact in fp32 and in bf16.  NaN in the K padding."""
    K = _K()
    n, H, W, C, k, s, p, Kp = _geom(g)
    Ho, Wo = _conv_out(H, W, k, s, p)
    d = _small_ints((n * Ho * Wo, Kp), 2)
    d[:, k * k * C:] = float("nan")
    ref = _col2im_ref(d, n, H, W, C, k, s, p)
    dd = d.to(dev)
    dx = K.col2im(dd, n, H, W, C, k, s, p).cpu()
    assert not torch.isnan(dx).any()
    assert torch.equal(dx.to(F64), ref)
    if g is BIG or g is COL2IM_LOOP:
        return
    # adjoint identity <im2col(x), d> == <x, col2im(d)>, exact in float64 on integers
    x = _small_ints((n * H * W, C), 3)
    col = K.im2col(x.to(dev), n, H, W, C, k, s, p, Kp).cpu()
    kk = k * k * C
    lhs = (col[:, :kk].to(F64) * d[:, :kk].to(F64)).sum().item()
    rhs = (x.to(F64) * dx.to(F64)).sum().item()
    assert lhs == rhs


@pytest.mark.parametrize("g", GEOMS[:-1], ids=_gid)
def test_col2im_random_within_one_ulp(dev, g):
    """At most k*k <= 49 fp32 additions, one rounding to bf16.  A = k*k * 2^-24 * sum |terms| (the fp32 summation bound)."""
    n, H, W, C, k, s, p, Kp = _geom(g)
    Ho, Wo = _conv_out(H, W, k, s, p)
    d = torch.randn(n * Ho * Wo, Kp, generator=_gen(4)).to(BF)
    ref = _col2im_ref(d, n, H, W, C, k, s, p)
    allowance = k * k * U32 * _col2im_ref(d, n, H, W, C, k, s, p, absolute=True)
    dx = _K().col2im(d.to(dev), n, H, W, C, k, s, p).cpu()
    worst, equal, beyond = _check_bf16(dx, ref, allowance)
    measured(NAME + "col2im_random", geom=_gid(g), worst_over_bar=worst, bit_equal=equal, beyond_plain_ulp=beyond)
    assert worst <= 1.0
    # pixels that no tap reads (stride 2) stay exactly zero
    taps = _col2im_ref(torch.ones(n * Ho * Wo, Kp), n, H, W, C, k, s, p)
    assert (_bits(dx)[taps == 0] == 0).all()
    if k == 1 and s == 2:
        dx4 = dx.view(n, H, W, C)
        assert (taps == 0).view(n, H, W, C)[:, 1::2].all() and (taps == 0).view(n, H, W, C)[:, :, 1::2].all()
        assert (_bits(dx4[:, 1::2]) == 0).all() and (_bits(dx4[:, :, 1::2]) == 0).all()


# ---- 3. max pool ----------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 9, 11, 64), (2, 8, 8, 64), (1, 1, 48, 64), (3, 2, 2, 8), (2, 112, 112, 64)]


def _pool_ref(x, n, H, W, C):
    y = F.max_pool2d(x.view(n, H, W, C).permute(0, 3, 1, 2).float(), 3, 2, 1)
    return y.permute(0, 2, 3, 1).reshape(-1, C).to(BF)                             # a max of bf16 values is a bf16 value


@pytest.mark.parametrize("kind", ["normal", "all_negative", "constant", "negative_constant"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_bit_exact(dev, shape, kind):
    n, H, W, C = shape
    x = torch.randn(n * H * W, C, generator=_gen(5))
    if kind == "all_negative":
        x = -x.abs() - 0.5                  # a zero-valued padding pixel would win every border window
    elif kind == "constant":
        x = torch.full_like(x, 1.5)
    elif kind == "negative_constant":
        x = torch.full_like(x, -2.0)
    x = x.to(BF)
    y = _K().maxpool3x3s2(x.to(dev), n, H, W, C).cpu()
    assert torch.equal(_bits(y), _bits(_pool_ref(x, n, H, W, C)))


def test_maxpool_grid_stride_loop(dev):
    """Output vectors > 16384 * 256, so the kernel's grid-stride loop runs more than once.  One image row keeps the input at
    twice the output (not four times), and small integers are cheap to draw and exact in bf16."""
    n, H, W, C = 1, 1, 131200, 512
    assert (W // 2) * C // 8 > 16384 * 256
    x = torch.randint(-120, 121, (W, C), generator=_gen(5), dtype=torch.int8).to(BF)
    y = _K().maxpool3x3s2(x.to(dev), n, H, W, C).cpu()
    xp = torch.cat([x[:1], x, x[-1:]])                       # repeating the edge pixel never changes a window's maximum
    ref = torch.maximum(torch.maximum(xp[0:W:2], xp[1:W + 1:2]), xp[2:W + 2:2])
    assert torch.equal(_bits(y), _bits(ref))


# ---- 4. batch norm forward -------------------------------------------------------------------------------------------------------
BN_SHAPES = [(63, 64), (64, 64), (65, 64), (1000, 8), (777, 24), (300, 200), (4096, 2048), (65537, 8), (65537, 64)]
BN_SMALL = [(63, 64), (64, 64), (65, 64), (1000, 8), (777, 24), (300, 200)]


def _bn_inputs(M, C, seed=6):
    g = _gen(seed + M + C)
    x = (torch.randn(M, C, generator=g) * 1.5 + torch.randn(C, generator=g) * 0.7).to(BF)
    res = torch.randn(M, C, generator=g).to(BF)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    rm = torch.randn(C, generator=g) * 0.2
    rv = torch.rand(C, generator=g) + 0.5
    return x, res, gamma, beta, rm, rv


def _stats64(x):
    x64 = x.to(F64)
    mu = x64.mean(0)
    var = ((x64 - mu) ** 2).mean(0)          # two-pass, float64
    return x64, mu, var, 1.0 / torch.sqrt(var + EPS)


def _y_ref(x64, mu, rs, gamma, beta, res, relu):
    """float64 y and the fp32-evaluation allowance A = 8 * 2^-24 * (|x scale| + |mean scale| + |beta| + |residual|): the kernel
    rounds mean, rstd, scale and shift to fp32 and evaluates fma(x, scale, shift) + residual in fp32."""
    sc = gamma.to(F64) * rs
    y = (x64 - mu) * sc + beta.to(F64)
    a = (x64 * sc).abs() + (mu * sc).abs() + beta.to(F64).abs()
    if res is not None:
        y = y + res.to(F64)
        a = a + res.to(F64).abs()
    return (y.clamp_min(0) if relu else y), 8 * U32 * a


@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batchnorm_fwd_train(dev, shape):
    """mean / rstd / running buffers: the kernel accumulates in fp64 and rounds each fp32 output once, so the bar is one fp32
    ulp (2^-23 relative; for the running buffers, of the two terms that are added)."""
    K = _K()
    M, C = shape
    x, res, gamma, beta, rm, rv = _bn_inputs(M, C)
    x64, mu, var, rs = _stats64(x)
    xd, resd, gd, bd = x.to(dev), res.to(dev), gamma.to(dev), beta.to(dev)
    rm_ref = (1 - MOM32) * rm.to(F64) + MOM32 * mu
    rv_ref = (1 - MOM32) * rv.to(F64) + MOM32 * var * (M / (M - 1))
    rm_tol = 2 * U32 * ((1 - MOM32) * rm.to(F64).abs() + MOM32 * mu.abs())
    rv_tol = 2 * U32 * rv_ref
    mean_tol = 2 * U32 * mu.abs() + 2.0 ** -40 * x64.abs().mean(0)
    first = True
    for use_res in (False, True):
        for relu in (False, True):
            rmd, rvd = rm.to(dev, copy=True), rv.to(dev, copy=True)
            y, mean, rstd = K.batchnorm_fwd(xd, gd, bd, rmd, rvd, True, EPS, MOM, residual=resd if use_res else None, relu=relu)
            e_mean = ((mean.cpu().to(F64) - mu).abs() / mean_tol).max().item()
            e_rstd = ((rstd.cpu().to(F64) - rs).abs() / rs).max().item()
            e_rm = ((rmd.cpu().to(F64) - rm_ref).abs() / rm_tol).max().item()
            e_rv = ((rvd.cpu().to(F64) - rv_ref).abs() / rv_tol).max().item()
            yref, allowance = _y_ref(x64, mu, rs, gamma, beta, res if use_res else None, relu)
            worst, equal, beyond = _check_bf16(y.cpu(), yref, allowance)
            if first:
                measured(NAME + "batchnorm_fwd_train", shape=f"{M}x{C}", mean_over_bar=e_mean, rstd_rel=e_rstd,
                         running_mean_over_bar=e_rm, running_var_over_bar=e_rv)
                first = False
            measured(NAME + "batchnorm_fwd_train_y", shape=f"{M}x{C}", residual=int(use_res), relu=int(relu),
                     worst_over_bar=worst, bit_equal=equal, beyond_plain_ulp=beyond)
            assert e_mean <= 1.0 and e_rstd <= 2 * U32 and e_rm <= 1.0 and e_rv <= 1.0, (e_mean, e_rstd, e_rm, e_rv)
            assert worst <= 1.0, (use_res, relu, worst)


@pytest.mark.parametrize("shape", BN_SMALL + [(65537, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batchnorm_fwd_eval(dev, shape):
    K = _K()
    M, C = shape
    x, res, gamma, beta, rm, rv = _bn_inputs(M, C)
    x64 = x.to(F64)
    rs = 1.0 / torch.sqrt(rv.to(F64) + EPS)
    rmd, rvd = rm.to(dev, copy=True), rv.to(dev, copy=True)
    for use_res in (False, True):
        for relu in (False, True):
            # train = False: no sum / sumsq buffers exist, the wrapper hands the kernel null pointers for them
            y, mean, rstd = K.batchnorm_fwd(x.to(dev), gamma.to(dev), beta.to(dev), rmd, rvd, False, EPS, MOM,
                                            residual=res.to(dev) if use_res else None, relu=relu)
            assert torch.equal(rmd.cpu().view(torch.int32), rm.view(torch.int32))          # untouched, bit for bit
            assert torch.equal(rvd.cpu().view(torch.int32), rv.view(torch.int32))
            assert torch.equal(mean.cpu().view(torch.int32), rm.view(torch.int32))
            e_rstd = ((rstd.cpu().to(F64) - rs).abs() / rs).max().item()
            yref, allowance = _y_ref(x64, rm.to(F64), rs, gamma, beta, res if use_res else None, relu)
            worst, equal, beyond = _check_bf16(y.cpu(), yref, allowance)
            measured(NAME + "batchnorm_fwd_eval", shape=f"{M}x{C}", residual=int(use_res), relu=int(relu), rstd_rel=e_rstd,
                     worst_over_bar=worst, bit_equal=equal, beyond_plain_ulp=beyond)
            assert e_rstd <= 2 * U32
            assert worst <= 1.0


def test_bn_apply_grid_stride_loop(dev):
    """(16400, 2048): more than 16384 * 256 vectors, so bn_apply's grid-stride loop runs more than once.  scale / shift are given."""
    from mmgclip._hip import call, ptr, stream
    M, C = 16400, 2048
    assert M * C // 8 > 16384 * 256
    g = _gen(7)
    x = torch.randn(M, C, generator=g).to(BF)
    res = torch.randn(M, C, generator=g).to(BF)
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g)
    xd, resd, scd, shd = x.to(dev), res.to(dev), scale.to(dev), shift.to(dev)      # named: a raw pointer keeps no tensor alive
    y = torch.full((M, C), float("nan"), device=dev, dtype=BF)
    call("mmg_bn_apply", ptr(xd), ptr(scd), ptr(shd), ptr(resd), ptr(y), M, C, 1, stream())
    y = y.cpu()
    del xd, resd, scd, shd
    # in fp32-sized pieces: y = relu(x scale + shift + res); A = 4 * 2^-24 * sum |terms| (one fma, one add)
    worst, equal = 0.0, 0.0
    for r0 in range(0, M, 4100):
        sl = slice(r0, r0 + 4100)
        xs = x[sl].to(F64) * scale.to(F64)
        ref = (xs + shift.to(F64) + res[sl].to(F64)).clamp_min(0)
        allowance = 4 * U32 * (xs.abs() + shift.to(F64).abs() + res[sl].to(F64).abs())
        w, e, _ = _check_bf16(y[sl], ref, allowance)
        worst, equal = max(worst, w), equal + e * ref.shape[0] / M
    measured(NAME + "bn_apply_grid_stride_loop", worst_over_bar=worst, bit_equal=equal)
    assert worst <= 1.0


COND_SHAPES = [(4096, 64), (65537, 8), (65537, 64)]
COND_RATIOS = [0, 1, 4, 16, 32]
COND_BAR = 2.0 ** -12


@pytest.mark.parametrize("shape", COND_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batchnorm_variance_conditioning(dev, shape):
    """Inputs 0.25 randn + r 0.25 (bf16) for r = mean/std in {0, 1, 4, 16, 32}: rstd, and the batch variance that enters
    running_var, within 2^-12 (relative) of float64 at every ratio.  A bf16 activation carries half an ulp = 2^-9 of rounding;
    eight times below that the statistic cannot move an output, and running_var is fp32 state that is checkpointed.

    The kernel's and torch's fp32 two-pass x.var(0) errors are both recorded (worst channel) whether the bar is met or not.
    Why the sums are fp64: with fp32 sums, fp32 atomics and sumsq/M - mean^2 in fp32, a plain sequential fp32 summation of the
    same inputs on the CPU gives rstd errors of 2e-3 ... 1e-1 at r = 16 and 32; fp64 sums leave one fp32 rounding (6e-8)."""
    K = _K()
    M, C = shape
    std = 0.25
    failures = []
    for r in COND_RATIOS:
        x = (std * torch.randn(M, C, generator=_gen(100 + r)) + r * std).to(BF)
        x64, mu, var, rs = _stats64(x)
        rmd, rvd = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        _, mean, rstd = K.batchnorm_fwd(x.to(dev), torch.ones(C, device=dev), torch.zeros(C, device=dev), rmd, rvd, True, EPS, MOM)
        var_k = rvd.cpu().to(F64) / MOM32 * ((M - 1) / M)              # running_var started at 0: momentum * unbiased variance
        e_rstd = ((rstd.cpu().to(F64) - rs).abs() / rs).max().item()
        e_var = ((var_k - var).abs() / var).max().item()
        e_mean = ((mean.cpu().to(F64) - mu).abs() / torch.sqrt(var)).max().item()
        vt = x.float().var(0, unbiased=False).to(F64)                  # what fp32 can do: torch's two-pass fp32 variance
        t_var = ((vt - var).abs() / var).max().item()
        t_rstd = ((1.0 / torch.sqrt(vt + EPS) - rs).abs() / rs).max().item()
        measured(NAME + "batchnorm_variance_conditioning", shape=f"{M}x{C}", ratio=r, kernel_rstd_rel=e_rstd, kernel_var_rel=e_var,
                 kernel_mean_err_in_std=e_mean, torch_fp32_rstd_rel=t_rstd, torch_fp32_var_rel=t_var, bar=COND_BAR)
        print(f"{M}x{C} r={r}: rstd {e_rstd:.2e} var {e_var:.2e} (torch fp32 two-pass: rstd {t_rstd:.2e} var {t_var:.2e})")
        if not (e_rstd <= COND_BAR and e_var <= COND_BAR):
            failures.append((r, e_rstd, e_var))
    assert not failures, f"(ratio, rstd rel, var rel) above 2^-12 = {COND_BAR:.2e}: {failures}"


# ---- 5. batch norm backward ------------------------------------------------------------------------------------------------------
# the small forward shapes, plus one row phase per column group (C = 2048) and rows_per_block above 64 (M > 1024 * 64)
BWD_SHAPES = BN_SMALL + [(130, 2048), (65537, 8)]


def _bwd_case(M, C, relu, use_res):
    """Inputs, the bf16 forward output `out` (with exact zeros from the ReLU), and the float64 autograd reference."""
    x, res, gamma, beta, _, _ = _bn_inputs(M, C, seed=8)
    dy = torch.randn(M, C, generator=_gen(9 + M)).to(BF)
    x64, mu, var, rs = _stats64(x)
    out = mask = None
    if relu:
        yref, _ = _y_ref(x64, mu, rs, gamma, beta, res if use_res else None, True)
        out = yref.to(BF)
        assert (out == 0).any() and (out > 0).any()
        mask = out > 0
    xa = x64.clone().requires_grad_(True)
    ga, ba = gamma.to(F64).requires_grad_(True), beta.to(F64).requires_grad_(True)
    ra = res.to(F64).requires_grad_(True)
    y = F.batch_norm(xa, None, None, ga, ba, True, 0.0, EPS)
    if use_res:
        y = y + ra
    # the ReLU's mask is the layer's own bf16 output, as in the tower; a masked element is +0 whatever dy's sign
    g64 = torch.where(mask, dy.to(F64), torch.zeros((), dtype=F64)) if relu else dy.to(F64)
    (y * g64).sum().backward()
    ref = dict(dx=xa.grad, dgamma=ga.grad, dbeta=ba.grad, dres=g64)
    # reference-side calibration of the two fp32 column reductions: per-column terms, a sequential fp32 sum against float64
    xh = (x64 - mu) * rs
    tol = {}
    for name, terms in (("sum_g", g64), ("sum_gx", g64 * xh)):
        t = terms.numpy()
        exact = t.sum(0)
        seq = np.cumsum(t.astype(np.float32), axis=0, dtype=np.float32)[-1].astype(np.float64)
        sabs = np.abs(t).sum(0)
        kappa = float((np.abs(seq - exact) / sabs).max())            # worst column, relative to sum |terms|
        tol[name] = torch.from_numpy(max(4 * kappa, 4 * 2 * U32) * sabs)        # x4: the atomics' order is free; floor: 4 fp32 ulps
        tol[name + "_calibration"] = kappa
    # the kernel's xhat comes from mean / rstd rounded to fp32: |delta xhat| <= 2^-24 (|x| + 2 |mean|) rstd, inside sum_gx too
    dxh = U32 * (x64.abs() + 2 * mu.abs()) * rs
    tol["sum_gx"] = tol["sum_gx"] + (g64.abs() * dxh).sum(0)
    grs = (gamma.to(F64) * rs).abs()
    sg, sgx = ref["dbeta"].detach().abs(), ref["dgamma"].detach().abs()
    # dx = gamma rstd (g - sum_g / M - xhat sum_gx / M) in fp32: the two sums' own bars, xhat's rounding, and 8 * 2^-24 of the |terms|
    tol["dx"] = grs / M * (tol["sum_g"] + xh.abs() * tol["sum_gx"] + dxh * sgx) + 8 * U32 * grs * (g64.abs() + sg / M + xh.abs() * sgx / M)
    return dict(x=x, dy=dy, out=out, gamma=gamma, mean=mu.float(), rstd=rs.float()), ref, tol


@pytest.mark.parametrize("mode", ["relu_res", "relu", "plain"])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batchnorm_bwd(dev, shape, mode):
    K = _K()
    M, C = shape
    relu, use_res = mode != "plain", mode == "relu_res"
    inp, ref, tol = _bwd_case(M, C, relu, use_res)
    d = {k: (v.to(dev) if v is not None else None) for k, v in inp.items()}
    g = _gen(10)
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)          # accumulated into: start non-zero
    # before + sum, added once more in fp32: one more ulp of the larger of the two
    tol_dg = tol["sum_gx"] + 2 * U32 * (dg0.to(F64).abs() + ref["dgamma"].abs())
    tol_db = tol["sum_g"] + 2 * U32 * (db0.to(F64).abs() + ref["dbeta"].abs())
    for attempt in (0, 1):                   # the atomics are unordered: both calls must stay inside the same bars
        dgd, dbd = dg0.to(dev, copy=True), db0.to(dev, copy=True)
        dx, dres = K.batchnorm_bwd(d["dy"], d["x"], d["out"], d["mean"], d["rstd"], d["gamma"], dgd, dbd, want_dres=use_res)
        e_dg = ((dgd.cpu().to(F64) - (dg0.to(F64) + ref["dgamma"])).abs() / tol_dg).max().item()
        e_db = ((dbd.cpu().to(F64) - (db0.to(F64) + ref["dbeta"])).abs() / tol_db).max().item()
        worst, equal, beyond = _check_bf16(dx.cpu(), ref["dx"], tol["dx"])
        measured(NAME + "batchnorm_bwd", shape=f"{M}x{C}", mode=mode, attempt=attempt, dgamma_over_bar=e_dg, dbeta_over_bar=e_db,
                 sum_g_calibration=tol["sum_g_calibration"], sum_gx_calibration=tol["sum_gx_calibration"],
                 dx_worst_over_bar=worst, dx_bit_equal=equal, dx_beyond_plain_ulp=beyond)
        assert e_dg <= 1.0 and e_db <= 1.0, (e_dg, e_db)
        assert worst <= 1.0
        if use_res:
            assert torch.equal(_bits(dres.cpu()), _bits(ref["dres"].to(BF)))      # the masked dy, bit for bit
        else:
            assert dres is None                                                   # nothing is allocated, nothing written
    # a null pair skips the parameter gradients; dx is the same
    dx2, _ = K.batchnorm_bwd(d["dy"], d["x"], d["out"], d["mean"], d["rstd"], d["gamma"], None, None)
    assert _check_bf16(dx2.cpu(), ref["dx"], tol["dx"])[0] <= 1.0


def test_batchnorm_bwd_rejects_half_a_gradient_pair(dev):
    from mmgclip import _hip
    from mmgclip._hip import ptr, stream
    M, C = 64, 64
    z = torch.zeros(M, C, device=dev, dtype=BF)
    f = torch.ones(C, device=dev)
    before = f.clone()
    lib = _hip.load()
    for dgamma, dbeta in ((f, None), (None, f)):
        rc = lib.mmg_bn_bwd_apply(ptr(z), ptr(z), None, ptr(f), ptr(f), ptr(f), ptr(f), ptr(f), M, C, ptr(z), None, ptr(dgamma),
                                  ptr(dbeta), stream())
        assert rc != 0
        assert "dgamma and dbeta go together" in _hip.last_error()
    assert torch.equal(f, before)
