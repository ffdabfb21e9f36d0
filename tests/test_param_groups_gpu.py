"""AdamW over an arena in several param groups, one launch (csrc/adamw_groups.hip, optim.FusedAdamW): the kernel against float64 numpy,
against itself launched per tensor (bitwise) and against the two existing AdamW kernels, the guard, and the optimizer / experiment
paths against torch.optim.AdamW built from the same groups."""
import copy

import numpy as np
import pytest
import torch

from tests.test_grad_clip_gpu import ATOL, LOOSE, LR, RTOL, SHAPES, WD, _close, _grad_values, _params, _set_grads, _state

pytestmark = pytest.mark.gpu
B1, B2, EPS = 0.9, 0.999, 1e-8
GRID_CAP, THREADS, PER_LANE = 2048, 256, 4                     # csrc/adamw_groups.hip: AG_MAX_WGS, AG_THREADS, one float4 per lane and trip
SIZES = [64, 192, 64 * 33, GRID_CAP * THREADS * PER_LANE + 192]  # a quarter wave; one wave in 3 groups; 33 chunks; one full grid-stride trip + 3 chunks
GROUP_LR = [LR, LR * 0.5, LR * 0.25, LR * 2.0]                  # the 4 groups of the optimizer tests
GROUP_WD = [WD, 0.0, 1e-2, 0.0]


def _f32(x):
    return float(np.float32(x))


def _kernel_case(n, seed=0):
    """Host inputs for n elements: groups alternating chunk by chunk, lr over 1e-6 ... 1e-2, weight decay 0 in every second group, and
    the tail of some chunks zero in p, g, m, v (an arena's padding gap)."""
    rng = np.random.default_rng(seed + n % 9973)
    n_groups = {64: 1, 192: 3}.get(n, 5)
    lrs = [_f32(x) for x in np.logspace(-6, -2, n_groups)] if n_groups > 1 else [_f32(1e-2)]
    wds = [_f32(1e-2) if k % 2 == 0 else 0.0 for k in range(n_groups)]
    cmap = (np.arange(n // 64) % n_groups).astype(np.uint8)
    p = rng.standard_normal(n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)         # the first three steps of a fresh state, as in test_adamw_matches_torch
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    gap = np.zeros(n, dtype=bool)
    for c in range(0, n // 64, 2):
        gap[c * 64 + 50:(c + 1) * 64] = True                        # 14 elements of padding behind a 50-element tensor
    for a in [p, m, v] + gs:
        a[gap] = 0.0
    return lrs, wds, cmap, p, m, v, gs, gap


@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_float64_numpy(dev, n):
    """The same update per element in float64, with the chunk's lr / wd and the fp32 hyper-parameter values the entry point takes;
    test_adamw_matches_torch's bars, over 3 steps."""
    from mmgclip import kernels as K
    lrs, wds, cmap, p, m, v, gs, gap = _kernel_case(n)
    lr_e, wd_e = np.repeat(np.array(lrs)[cmap], 64), np.repeat(np.array(wds)[cmap], 64)
    b1, b2, eps = _f32(B1), _f32(B2), _f32(EPS)
    rp, rm, rv = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    dp, dm, dv = (torch.from_numpy(a.copy()).to(dev) for a in (p, m, v))
    dmap = torch.from_numpy(cmap).to(dev)
    for t, g in enumerate(gs, start=1):
        K.adamw_step_groups(dp, torch.from_numpy(g.copy()).to(dev), dm, dv, dmap, lrs, wds, B1, B2, EPS, t)
        g64 = g.astype(np.float64)
        rp *= 1.0 - lr_e * wd_e
        rm = b1 * rm + (1.0 - b1) * g64
        rv = b2 * rv + (1.0 - b2) * g64 * g64
        rp -= (lr_e / (1.0 - b1 ** t)) * rm / (np.sqrt(rv) / np.sqrt(1.0 - b2 ** t) + eps)
    for name, got, want in (("p", dp, rp), ("m", dm, rm), ("v", dv, rv)):
        got = got.cpu().numpy()
        err = np.abs(got - want)
        print(f"n={n} {name}: max abs err {err.max():.3e}, max err / (atol + rtol |ref|) {(err / (ATOL + RTOL * np.abs(want))).max():.3f}")
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
        assert not got[gap].any()                                   # the padding gaps stayed exactly zero
    assert float(np.abs(dp.cpu().numpy() - p).max()) > 1e-3         # (and the largest lr moved its chunks visibly)


# ---- the hand-made arena of tests/test_grad_clip_gpu.py, 4 groups alternating tensor by tensor ----------------------------------------
def _arena_case(dev, seed=0):
    from mmgclip.optim import build_chunk_map
    arena, _ = _params(dev, seed)
    slots = [i % 4 for i in range(len(SHAPES))]
    for n, val in zip(arena.names, _grad_values(40 + seed, 1.0)):
        arena.g(n).copy_(val)
    g = torch.Generator().manual_seed(7 + seed)
    m, v = torch.zeros(arena.size), torch.zeros(arena.size)
    for n, p in zip(arena.names, arena.params):                     # moments with the gaps zero, as FusedAdamW keeps them
        o = arena.offsets[n]
        m[o:o + p.numel()] = torch.randn(p.numel(), generator=g) * 0.1
        v[o:o + p.numel()] = torch.rand(p.numel(), generator=g) * 0.01
    return arena, slots, build_chunk_map(arena, slots).to(dev), m.to(dev), v.to(dev)


def _spans(arena):
    """(index, first element, padded length) of every tensor of the arena."""
    return [(i, arena.offsets[n], (p.numel() + 63) // 64 * 64) for i, (n, p) in enumerate(zip(arena.names, arena.params))]


def _guard(dev, coef=0.37, apply=1.0, skipped=1):
    return torch.tensor([50.0, coef, apply, 0.0], device=dev), torch.tensor([skipped], device=dev, dtype=torch.int32)


@pytest.mark.parametrize("guarded", [False, True])
def test_one_launch_equals_the_same_kernel_per_tensor_bitwise(dev, guarded):
    """Position independence: what an element becomes depends on its group's values alone, not on where in the launch it sits."""
    from mmgclip import kernels as K
    arena, slots, cmap, m0, v0 = _arena_case(dev)
    clip, skipped = _guard(dev) if guarded else (None, None)
    p, m, v = arena.data.clone(), m0.clone(), v0.clone()
    K.adamw_step_groups(p, arena.grad, m, v, cmap, GROUP_LR, GROUP_WD, B1, B2, EPS, 5, clip, skipped)
    q, mq, vq = arena.data.clone(), m0.clone(), v0.clone()
    zero = torch.zeros(arena.size // 64, device=dev, dtype=torch.uint8)
    for i, o, ln in _spans(arena):
        s = slots[i]
        K.adamw_step_groups(q[o:o + ln], arena.grad[o:o + ln], mq[o:o + ln], vq[o:o + ln], zero[:ln // 64], [GROUP_LR[s]], [GROUP_WD[s]],
                            B1, B2, EPS, 5, clip, skipped)
    assert torch.equal(p, q) and torch.equal(m, mq) and torch.equal(v, vq)
    assert not torch.equal(p, arena.data) and torch.isfinite(p).all()


@pytest.mark.parametrize("guarded", [False, True])
def test_one_launch_against_the_existing_kernels_per_tensor(dev, guarded):
    """mmg_adamw_step / mmg_adamw_step_guarded per tensor with the group's values: the same arithmetic, expected bit-equal; held to
    the project's bars and the outcome printed."""
    from mmgclip import kernels as K
    arena, slots, cmap, m0, v0 = _arena_case(dev, seed=1)
    clip, skipped = _guard(dev) if guarded else (None, None)
    p, m, v = arena.data.clone(), m0.clone(), v0.clone()
    K.adamw_step_groups(p, arena.grad, m, v, cmap, GROUP_LR, GROUP_WD, B1, B2, EPS, 5, clip, skipped)
    q, mq, vq = arena.data.clone(), m0.clone(), v0.clone()
    for i, o, ln in _spans(arena):
        s, args = slots[i], (q[o:o + ln], arena.grad[o:o + ln], mq[o:o + ln], vq[o:o + ln], None)
        if guarded:
            K.adamw_step_guarded(*args, GROUP_LR[s], B1, B2, EPS, GROUP_WD[s], 5, clip, skipped)
        else:
            K.adamw_step(*args, GROUP_LR[s], B1, B2, EPS, GROUP_WD[s], 5)
    print(f"grouped launch vs {'mmg_adamw_step_guarded' if guarded else 'mmg_adamw_step'} per tensor: bit-equal = "
          f"{torch.equal(p, q) and torch.equal(m, mq) and torch.equal(v, vq)}")
    for a, b in ((p, q), (m, mq), (v, vq)):
        _close(a, b)


def test_guard_holds_every_group_back_and_the_clock_clamps_at_one(dev):
    from mmgclip import kernels as K
    arena, slots, cmap, m0, v0 = _arena_case(dev, seed=2)
    clip, skipped = _guard(dev, apply=0.0)
    p, m, v = arena.data.clone(), m0.clone(), v0.clone()
    K.adamw_step_groups(p, arena.grad, m, v, cmap, GROUP_LR, GROUP_WD, B1, B2, EPS, 5, clip, skipped)
    assert torch.equal(p, arena.data) and torch.equal(m, m0) and torch.equal(v, v0)       # clip[2] == 0: no group moved, bit for bit
    # a chunk whose group index is not a group of the launch is left untouched, its neighbours are not
    few = cmap.clone()
    few[0] = 9
    K.adamw_step_groups(p, arena.grad, m, v, few, GROUP_LR, GROUP_WD, B1, B2, EPS, 5)
    assert torch.equal(p[:64], arena.data[:64]) and torch.equal(m[:64], m0[:64]) and not torch.equal(p[64:], arena.data[64:])
    # step 2 with 5 steps skipped: t = -3 is clamped to 1, the first Adam step
    runs = []
    for step, sk in ((2, 5), (1, 0)):
        clip, skipped = _guard(dev, skipped=sk)
        p, m, v = arena.data.clone(), m0.clone(), v0.clone()
        K.adamw_step_groups(p, arena.grad, m, v, cmap, GROUP_LR, GROUP_WD, B1, B2, EPS, step, clip, skipped)
        runs.append((p, m, v))
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and torch.isfinite(runs[0][0]).all()


# ---- optim.FusedAdamW with 4 groups against torch.optim.AdamW ---------------------------------------------------------------------------
def _grouped(params, betas=None):
    groups = [dict(params=[], lr=GROUP_LR[k], weight_decay=GROUP_WD[k], name=f"g{k}") for k in range(4)]
    for i, p in enumerate(params):
        groups[i % 4]["params"].append(p)                           # interleaved over the arena, and on over the loose tensors
    if betas is not None:
        groups[2]["betas"] = betas
    return groups


def _pair(dev, seed=0, betas=None, **kw):
    """(FusedAdamW over the arena + loose tensors in 4 groups, arena, loose, its parameters, torch.optim.AdamW over copies in the same groups, the copies)."""
    from mmgclip.optim import FusedAdamW
    arena, loose = _params(dev, seed)
    mine = arena.params + loose
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    return (FusedAdamW(_grouped(mine, betas), lr=LR, weight_decay=WD, **kw), arena, loose, mine,
            torch.optim.AdamW(_grouped(theirs, betas), lr=LR, weight_decay=WD), theirs)


def _count_launches(monkeypatch):
    from mmgclip import kernels as K
    seen = []
    for name in ("adamw_step", "adamw_step_guarded", "adamw_step_groups"):
        def wrapped(p, *a, _fn=getattr(K, name), _name=name, **k):
            seen.append((_name, p.data_ptr(), p.numel()))
            return _fn(p, *a, **k)
        monkeypatch.setattr(K, name, wrapped)
    return seen


def _arena_launches(seen, arena):
    lo, hi = arena.data.data_ptr(), arena.data.data_ptr() + 4 * arena.size
    return [s for s in seen if lo <= s[1] < hi]


@pytest.mark.parametrize("max_grad_norm", [None, 1.0])
def test_four_groups_follow_torch_with_one_launch_for_the_arena(dev, monkeypatch, max_grad_norm):
    kw = {} if max_grad_norm is None else dict(max_grad_norm=max_grad_norm)
    opt, arena, loose, mine, ref, theirs = _pair(dev, **kw)
    schedule = [torch.optim.lr_scheduler.LambdaLR(o, lambda e: 1.0 / (1.0 + 0.5 * e)) for o in (opt, ref)]
    seen = _count_launches(monkeypatch)
    n_elem = sum(p.numel() for p in mine)
    for step in range(5):
        values = _grad_values(170 + step, 1.0 if max_grad_norm is None else 50.0 / n_elem ** 0.5)
        _set_grads(arena, loose, values)
        for p, val in zip(theirs, values):
            p.grad = val.to(dev).clone()
        if max_grad_norm is not None:
            want = float(torch.nn.utils.clip_grad_norm_(theirs, max_grad_norm))       # one norm over all groups
        del seen[:]
        opt.step()
        ref.step()
        # THE point: the arena, spread over 4 groups, goes out as exactly one launch (per tensor it would be 20), the loose tensors one each
        assert _arena_launches(seen, arena) == [("adamw_step_groups", arena.data.data_ptr(), arena.size)], seen
        assert len(seen) == 1 + len(LOOSE)
        if max_grad_norm is not None:
            got = opt.grad_norm.tolist()
            assert 40.0 < want < 60.0 and got[2] == 1.0 and got[1] < 0.03 and abs(got[0] - want) <= 1e-6 * want
        for s in schedule:
            s.step()
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in ref.param_groups]
    assert abs(opt.param_groups[0]["lr"] - LR / 3.5) < 1e-12 * LR    # the lrs did change between steps
    for a, b in zip(mine, theirs):
        _close(a, b)
    assert opt.skipped_steps() == 0 and int(opt.state[arena.params[0]]["step"]) == 5
    assert opt.state[arena.params[3]]["exp_avg"].data_ptr() == opt._flat[id(arena)]["m"].data_ptr() + 4 * arena.offsets["w3"]


def test_poisoned_step_leaves_the_grouped_state_as_if_it_never_came(dev):
    g1, g2 = _grad_values(191, 0.3), _grad_values(192, 0.3)
    poisoned = [v.clone() for v in _grad_values(194, 0.3)]
    poisoned[6].view(-1)[5] = float("nan")                          # inside the arena
    a, arena_a, loose_a, *_ = _pair(dev, max_grad_norm=1.0)
    b, arena_b, loose_b, *_ = _pair(dev, max_grad_norm=1.0)
    for values in (g1, poisoned, g2):
        _set_grads(arena_a, loose_a, values)
        a.step()
    for values in (g1, g2):
        _set_grads(arena_b, loose_b, values)
        b.step()
    assert all(torch.equal(x, y) for x, y in zip(_state(a, arena_a, loose_a), _state(b, arena_b, loose_b)))
    assert a.skipped_steps() == 1 and b.skipped_steps() == 0 and "chunk_map" in a._flat[id(arena_a)]
    assert all(float(s["step"]) == 2.0 for s in a.state_dict()["state"].values())


def test_single_group_keeps_todays_launch(dev, monkeypatch):
    from mmgclip.optim import FusedAdamW
    arena, loose = _params(dev)
    opt = FusedAdamW(arena.params + loose, lr=LR, weight_decay=WD)
    seen = _count_launches(monkeypatch)
    for step in range(2):
        _set_grads(arena, loose, _grad_values(60 + step, 1.0))
        opt.step()
    assert [s[0] for s in seen] == ["adamw_step"] * (2 * (1 + len(LOOSE)))
    assert _arena_launches(seen, arena) == [("adamw_step", arena.data.data_ptr(), arena.size)] * 2
    assert "chunk_map" not in opt._flat[id(arena)]


def test_mixed_betas_take_the_per_tensor_path_with_each_groups_values(dev, monkeypatch):
    opt, arena, loose, mine, ref, theirs = _pair(dev, betas=(0.8, 0.99))
    seen = _count_launches(monkeypatch)
    for step in range(2):
        values = _grad_values(80 + step, 1.0)
        _set_grads(arena, loose, values)
        for p, val in zip(theirs, values):
            p.grad = val.to(dev).clone()
        opt.step()
        ref.step()
    assert [s[0] for s in seen] == ["adamw_step"] * (2 * (len(SHAPES) + len(LOOSE)))
    for a, b in zip(mine, theirs):
        _close(a, b)


def test_checkpoint_round_trip_and_torch_interchange_with_groups(dev):
    g1, g2, g3, g4 = (_grad_values(s, 0.3) for s in (101, 102, 103, 104))
    a, arena_a, loose_a, mine_a, ref, theirs = _pair(dev)
    for values in (g1, g2):
        _set_grads(arena_a, loose_a, values)
        a.step()
    sd = a.state_dict()
    assert [g["name"] for g in sd["param_groups"]] == ["g0", "g1", "g2", "g3"] and len(sd["state"]) == len(SHAPES) + len(LOOSE)
    assert all(float(s["step"]) == 2.0 for s in sd["state"].values())
    # -> a fresh FusedAdamW over the same values and groups: the next step is bit-equal
    c, arena_c, loose_c, *_ = _pair(dev)
    with torch.no_grad():
        arena_c.data.copy_(arena_a.data)
        for pc, pa in zip(loose_c, loose_a):
            pc.copy_(pa)
        for pt, pa in zip(theirs, mine_a):
            pt.copy_(pa)
    c.load_state_dict(copy.deepcopy(sd))
    ref.load_state_dict(copy.deepcopy(sd))                            # -> torch.optim.AdamW built from the same groups
    for opt, arena, loose in ((a, arena_a, loose_a), (c, arena_c, loose_c)):
        _set_grads(arena, loose, g3)
        opt.step()
    assert all(torch.equal(x, y) for x, y in zip(_state(a, arena_a, loose_a), _state(c, arena_c, loose_c)))
    for p, val in zip(theirs, g3):
        p.grad = val.to(dev).clone()
    ref.step()
    for x, y in zip(mine_a, theirs):
        _close(x, y)
    # and back: torch's state dict into a fresh FusedAdamW, one more step on both
    back, arena_d, loose_d, mine_d, *_ = _pair(dev)
    with torch.no_grad():
        for pd, pt in zip(mine_d, theirs):
            pd.copy_(pt)
    back.load_state_dict(copy.deepcopy(ref.state_dict()))
    _set_grads(arena_d, loose_d, g4)
    back.step()
    for p, val in zip(theirs, g4):
        p.grad = val.to(dev).clone()
    ref.step()
    for x, y in zip(mine_d, theirs):
        _close(x, y)
    assert all(float(s["step"]) == 4.0 for s in back.state_dict()["state"].values())


# ---- the whole model through ClassifierExperiment ---------------------------------------------------------------------------------------
def test_whole_model_finetune_recipe_follows_the_torch_path(dev, tmp_path, monkeypatch):
    from tests.test_experiment_gpu import _delta_agreement, _experiment, _loader, _weights
    runs = {}
    for name, fused in (("fused", "true"), ("torch", "false")):
        exp = _experiment(str(tmp_path / name), ["optimizer=adamw_finetune", f"optimizer.config.fused={fused}",
                                                 "optimizer.config.learning_rate=5e-4"], _loader(steps=3, n=4))
        assert type(exp.optimizer).__name__ == ("FusedAdamW" if name == "fused" else "AdamW")
        assert len(exp.optimizer.param_groups) > 20
        w0 = _weights(exp)
        exp.scheduler.step()                      # leave the reference's lr-0 first epoch
        exp.scheduler.step()
        with monkeypatch.context() as mp_:
            seen = _count_launches(mp_)
            exp.train()                           # three steps
        if name == "fused":
            opt = exp.optimizer
            ia, ta = exp.model.image_encoder.arena, exp.model.text_encoder.arena
            for arena in (ia, ta):                # one AdamW launch per tower arena and step, and the towers were told
                assert _arena_launches(seen, arena) == [("adamw_step_groups", arena.data.data_ptr(), arena.size)] * 3
                assert arena.manual_version >= 3
            loose = [p for p in exp.model.parameters() if p.grad is not None and getattr(p, "_mmg_arena", None) is None]
            assert len(seen) == 3 * (2 + len(loose))
            assert opt.grad_norm.tolist()[2] == 1.0 and opt.skipped_steps() == 0 and int(opt.state[ia.params[0]]["step"]) == 3
        else:
            assert not seen
        runs[name] = (_weights(exp), w0)
    cos, ratio = _delta_agreement(runs["fused"][0], runs["torch"][0], runs["torch"][1])
    print(f"fine-tuning recipe, fused vs torch AdamW after 3 steps: movement cosine {cos:.4f}, norm ratio {ratio:.4f}")
    assert cos > 0.9 and 0.95 < ratio < 1.05, (cos, ratio)               # test_fused_adamw_built_before_first_forward_trains_the_towers' bars
