"""Gradient clipping by global norm and the non-finite-step guard on the device (csrc/grad_clip.hip, optim.FusedAdamW):
the norm against float64 numpy, the coefficient against torch's formula, the guard, and the optimizer / experiment / two-rank
paths against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW."""
import copy
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
SIZES = [1, 3, 255, 256, 257, 8191, 8193, (1 << 24) + 5]     # the last one: more than one grid-stride trip and a ragged tail
LR, WD = 5e-5, 1e-4                                           # tests/test_kernels_gpu.py::test_adamw_matches_torch's step and bars
RTOL, ATOL = 1e-6, 1e-7


@functools.lru_cache(maxsize=None)
def _host_values(n, seed=0):
    """n fp32 values of either sign with magnitudes spread over 1e-6 ... 1e3, and their norm in float64 (computed once, shared)."""
    rng = np.random.default_rng(1000 + seed + n % 9973)
    x = (10.0 ** rng.uniform(-6.0, 3.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    x.setflags(write=False)
    return x, float(np.sqrt(np.sum(x.astype(np.float64) ** 2)))


def _reduce(pieces, max_norm=None, skipped=None):
    """sumsq of every piece into one partials buffer + one finalize: (out fp32 [4] on the host, partials on the device)."""
    from mmgclip import kernels as K
    counts = [K.grad_sumsq_partials(g.numel()) for g in pieces]
    partials = torch.full((sum(counts),), -1.0, device=pieces[0].device, dtype=torch.float64)
    off = 0
    for g, c in zip(pieces, counts):
        K.grad_sumsq(g, partials, off, c)
        off += c
    out = torch.zeros(4, device=pieces[0].device)
    K.grad_clip_finalize(partials, off, max_norm, out, skipped)
    return out.cpu(), partials


@pytest.mark.parametrize("n", SIZES)
def test_norm_matches_float64_numpy(dev, n):
    x, ref = _host_values(n)
    g = torch.from_numpy(x.copy()).to(dev)
    out, partials = _reduce([g])
    norm = float(out[0])
    print(f"n={n}: norm {norm!r} ref {ref!r} rel {abs(norm - ref) / ref:.2e}")
    assert abs(norm - ref) <= 1e-6 * ref
    assert float(out[1]) == 1.0 and float(out[2]) == 1.0
    _, again = _reduce([g])
    assert torch.equal(partials, again)                       # same input, same bits
    assert abs(float(partials.sum().sqrt()) - ref) <= 1e-6 * ref


@pytest.mark.parametrize("n", [1, 3, 257, 8193])
def test_norm_of_a_four_byte_aligned_view(dev, n):
    x, ref = _host_values(n, seed=1)
    base = torch.zeros(n + 1, device=dev)
    base[0] = 1e6                                             # an element in front of the view that must not be read
    g = base[1:]
    g.copy_(torch.from_numpy(x.copy()))
    assert g.data_ptr() % 16 == 4 and g.is_contiguous()
    out, _ = _reduce([g])
    assert abs(float(out[0]) - ref) <= 1e-6 * ref


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 8198, 8192 * 3 + 5])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_element_is_counted_exactly_once(dev, n, shift):
    """All ones: the partials sum to n exactly, so one dropped or doubled head / body / tail element shows - at every alignment of the
    pointer inside a 16-byte line, with sentinels of 1000 on both sides of the view that must not be read."""
    base = torch.full((n + shift + 4,), 1000.0, device=dev)
    g = base[shift:shift + n]
    g.fill_(1.0)
    assert g.data_ptr() % 16 == 4 * shift
    out, partials = _reduce([g])
    assert float(partials.sum()) == float(n), (n, shift, partials.tolist())
    assert float(out[0]) == float(np.float32(np.sqrt(np.float64(n))))


def test_pieces_finalized_together_equal_the_norm_of_their_concatenation(dev):
    ns = [1, 257, 8193, 3, 70001]
    xs = [_host_values(n, seed=2 + i)[0] for i, n in enumerate(ns)]
    ref = float(np.sqrt(np.sum(np.concatenate(xs).astype(np.float64) ** 2)))
    pieces = [torch.from_numpy(x.copy()).to(dev) for x in xs]
    pieces[0] = pieces[0].reshape(())                         # a 0-d gradient (logit_scale)
    out, partials = _reduce(pieces)
    assert partials.numel() == 1 + 1 + 2 + 1 + 9 and (partials >= 0).all()       # every partial was written
    assert abs(float(out[0]) - ref) <= 1e-6 * ref
    one, _ = _reduce([torch.from_numpy(np.concatenate(xs)).to(dev)])
    assert abs(float(one[0]) - ref) <= 1e-6 * ref


def test_clip_coefficient(dev):
    x, _ = _host_values(8193, seed=7)
    g = torch.from_numpy(x.copy()).to(dev)
    norm = np.float32(_reduce([g])[0][0])
    for max_norm in (float(norm) * 2, float(norm) * 1.0000001 + 1e-3, 1e30):
        assert float(_reduce([g], max_norm)[0][1]) == 1.0, max_norm      # above the norm: exactly 1
    for max_norm in (float(norm) * 0.5, 1.0, 0.1, 1e-4, float(norm) * 0.999):
        coef = np.float32(_reduce([g], max_norm)[0][1])
        want = np.float32(max_norm) / (norm + np.float32(1e-6))          # torch.nn.utils.clip_grad_norm_, in fp32 as torch does it
        assert coef < 1.0 and abs(coef - want) <= np.spacing(want), (max_norm, coef, want)
    for max_norm in (0.0, float("inf"), None, -3.0):                     # "no clipping"
        out = _reduce([g], max_norm)[0]
        assert float(out[1]) == 1.0 and float(out[0]) == float(norm) and float(out[2]) == 1.0


def test_nonfinite_gradient_is_flagged_counted_and_not_applied(dev):
    from mmgclip import kernels as K
    na, nb = 1000, 8198                     # piece b starts 4 bytes past a 16-byte boundary: 3 head elements, 2048 float4, 3 tail elements
    a = torch.from_numpy(_host_values(na, seed=11)[0].copy()).to(dev)
    base = torch.zeros(nb + 1, device=dev)
    b = base[1:]
    b.copy_(torch.from_numpy(_host_values(nb, seed=12)[0].copy()))
    assert b.data_ptr() % 16 == 4
    skipped = torch.zeros(1, device=dev, dtype=torch.int32)
    p0 = torch.randn(na, device=dev)
    m0, v0 = torch.rand(na, device=dev) * 0.1, torch.rand(na, device=dev) * 0.01
    count = 0
    for bad in (float("nan"), float("inf"), float("-inf")):
        for piece, idx in ((a, 0), (b, nb - 1), (b, nb - 2), (b, 1)):         # first element, last element, inside the tail, inside the head
            keep = piece[idx].clone()
            piece[idx] = bad
            out, _ = _reduce([a, b], 1.0, skipped)
            count += 1
            assert float(out[2]) == 0.0 and int(skipped.item()) == count, (bad, idx, out)
            clip = out.to(dev)
            p, m, v, p16 = p0.clone(), m0.clone(), v0.clone(), torch.full((na,), 7.0, device=dev, dtype=BF)
            K.adamw_step_guarded(p, a, m, v, p16, 1e-2, 0.9, 0.999, 1e-8, 1e-2, 5, clip, skipped)
            assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0) and bool((p16 == 7.0).all())
            piece[idx] = keep                                                  # the same buffers with the bad value replaced
            out, _ = _reduce([a, b], 1.0, skipped)
            assert float(out[2]) == 1.0 and int(skipped.item()) == count and np.isfinite(float(out[0]))
    # and the good gradient does step (t = 5 - 12 skipped < 1 is clamped to 1)
    p, m, v, p16 = p0.clone(), m0.clone(), v0.clone(), torch.full((na,), 7.0, device=dev, dtype=BF)
    K.adamw_step_guarded(p, a, m, v, p16, 1e-2, 0.9, 0.999, 1e-8, 1e-2, 5, out.to(dev), skipped)
    assert not torch.equal(p, p0) and torch.equal(p16, p.to(BF)) and torch.isfinite(p).all()
    # skipped == None: the guard is off, a non-finite norm is neither counted nor held back
    a[0] = float("nan")
    out, _ = _reduce([a, b], 1.0, None)
    assert float(out[2]) == 0.0 and int(skipped.item()) == count


# ---- optim.FusedAdamW over a hand-made arena + loose tensors ---------------------------------------------------------------------
SHAPES = [(7,), (3, 5), (64,), (129,), (1,), (16, 16), (33,), (2, 3, 4), (100,), (5,), (64, 2), (17,), (256,), (9, 9), (1, 1), (31,),
          (48,), (3,), (65,), (128,)]
LOOSE = [(40, 12), (77,), ()]


def _params(dev, seed=0):
    """(arena of 20 small tensors - most of them leave padding gaps -, 3 loose parameters, one of them 0-d)."""
    from mmgclip.params import ParamArena
    g = torch.Generator().manual_seed(seed)
    named = [(f"w{i}", torch.nn.Parameter(torch.randn(s, generator=g))) for i, s in enumerate(SHAPES)]
    arena = ParamArena(named, dev)
    loose = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in LOOSE]
    return arena, loose


def _grad_values(seed, scale):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * scale for s in SHAPES + LOOSE]


def _set_grads(arena, loose, values):
    for n, p, val in zip(arena.names, arena.params, values):
        arena.g(n).copy_(val)
        p.grad = arena.g(n)
    for p, val in zip(loose, values[len(SHAPES):]):
        p.grad = val.to(p.device).clone()


def _optimizer(dev, seed=0, **kw):
    from mmgclip.optim import FusedAdamW
    arena, loose = _params(dev, seed)
    return FusedAdamW(arena.params + loose, lr=LR, weight_decay=WD, **kw), arena, loose


def _state(opt, arena, loose):
    fs = opt._flat[id(arena)]
    return [arena.data.clone(), fs["m"].clone(), fs["v"].clone()] + \
           [t.clone() for p in loose for t in (p.data, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]


def _close(a, b):
    np.testing.assert_allclose(a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy(), rtol=RTOL, atol=ATOL)


def test_inactive_clip_has_no_side_effects(dev):
    """max_grad_norm far above the norm: coefficient exactly 1, nothing skipped.  After the first step (beta^1 needs no pow) the
    guarded run is bit-equal to the unguarded one; later steps take beta^t from the device (fp64 repeated squaring, rounded once)
    instead of the host's powf, which is not bit-equal in general and is held to test_adamw_matches_torch's bars."""
    runs = {}
    for name, kw in (("guarded", dict(max_grad_norm=1e9)), ("plain", dict())):
        opt, arena, loose = _optimizer(dev, **kw)
        snaps = []
        for step in range(3):
            _set_grads(arena, loose, _grad_values(50 + step, 1.0))
            opt.step()
            snaps.append(_state(opt, arena, loose))
        runs[name] = snaps
        if name == "guarded":
            assert opt.grad_norm.tolist()[1:3] == [1.0, 1.0] and opt.skipped_steps() == 0
            assert len(opt._piece_sizes) == 4 and opt._piece_sizes[0] == arena.size        # the arena went in as one flat piece
        else:
            assert opt.grad_norm is None
    assert all(torch.equal(a, b) for a, b in zip(runs["guarded"][0], runs["plain"][0]))
    print("bit-equal after 3 steps:", all(torch.equal(a, b) for a, b in zip(runs["guarded"][2], runs["plain"][2])))
    for a, b in zip(runs["guarded"][2], runs["plain"][2]):
        _close(a, b)


def test_active_clip_follows_torch(dev):
    opt, arena, loose = _optimizer(dev, max_grad_norm=1.0)
    mine = arena.params + loose
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    ref = torch.optim.AdamW(theirs, lr=LR, weight_decay=WD)
    n_elem = sum(p.numel() for p in mine)
    for step in range(5):
        values = _grad_values(70 + step, 50.0 / n_elem ** 0.5)           # norm ~ 50
        _set_grads(arena, loose, values)
        for p, val in zip(theirs, values):
            p.grad = val.to(dev).clone()
        want = float(torch.nn.utils.clip_grad_norm_(theirs, 1.0))
        ref.step()
        opt.step()
        got = opt.grad_norm.tolist()
        print(f"step {step}: norm {got[0]!r} torch {want!r} coef {got[1]!r}")
        assert 40.0 < want < 60.0 and got[2] == 1.0 and got[1] < 0.03
        assert abs(got[0] - want) <= 1e-6 * want
    for a, b in zip(mine, theirs):
        _close(a, b)
    assert opt.skipped_steps() == 0


def test_skipped_step_does_not_advance_adams_clock(dev):
    g1, g2, g3 = _grad_values(91, 0.3), _grad_values(92, 0.3), _grad_values(93, 0.3)
    poisoned = [v.clone() for v in _grad_values(94, 0.3)]
    poisoned[6].view(-1)[5] = float("nan")                               # inside the arena
    a, arena_a, loose_a = _optimizer(dev, max_grad_norm=1.0)
    b, arena_b, loose_b = _optimizer(dev, max_grad_norm=1.0)
    for values in (g1, poisoned, g2):
        _set_grads(arena_a, loose_a, values)
        a.step()
    for values in (g1, g2):
        _set_grads(arena_b, loose_b, values)
        b.step()
    assert all(torch.equal(x, y) for x, y in zip(_state(a, arena_a, loose_a), _state(b, arena_b, loose_b)))
    assert a.skipped_steps() == 1 and b.skipped_steps() == 0 and a.grad_norm.tolist()[2] == 1.0
    assert int(a.state[arena_a.params[0]]["step"]) == 3                  # the host counters count step() calls ...
    sd = a.state_dict()
    assert len(sd["state"]) == len(SHAPES) + len(LOOSE)
    assert all(float(s["step"]) == 2.0 for s in sd["state"].values())    # ... the checkpoint holds Adam's clock
    assert all(float(s["step"]) == 2.0 for s in b.state_dict()["state"].values())
    # a fresh optimizer over the same values, loaded from that checkpoint, continues as the original does
    c, arena_c, loose_c = _optimizer(dev, max_grad_norm=1.0)
    with torch.no_grad():
        arena_c.data.copy_(arena_a.data)
        for pc, pa in zip(loose_c, loose_a):
            pc.copy_(pa)
    c.load_state_dict(copy.deepcopy(sd))                                 # (as from a checkpoint file: torch keeps the tensors it is handed)
    for opt, arena, loose in ((a, arena_a, loose_a), (c, arena_c, loose_c)):
        _set_grads(arena, loose, g3)
        opt.step()
    assert all(torch.equal(x, y) for x, y in zip(_state(a, arena_a, loose_a), _state(c, arena_c, loose_c)))
    assert c.skipped_steps() == 0 and all(float(s["step"]) == 3.0 for s in c.state_dict()["state"].values())
    assert all(float(s["step"]) == 3.0 for s in a.state_dict()["state"].values())
    # loading into the optimizer that skipped: its device count starts again, the clock is the loaded one
    a.load_state_dict(copy.deepcopy(sd))
    assert a.skipped_steps() == 0 and int(a.state[loose_a[0]]["step"]) == 2


def test_parameter_that_joins_after_a_skipped_step_starts_its_own_clock(dev):
    """A parameter whose first gradient arrives after guarded steps have run (one of them skipped): its counter starts at the skipped
    count - the one read-back `step()` can make - so its first update is a first Adam step and its checkpoint says step 1."""
    from mmgclip.optim import FusedAdamW
    torch.manual_seed(3)
    w, q = torch.nn.Parameter(torch.randn(300, device=dev)), torch.nn.Parameter(torch.randn(50, device=dev))
    alone = torch.nn.Parameter(q.detach().clone())
    opt = FusedAdamW([w, q], lr=LR, weight_decay=WD, max_grad_norm=1e9)
    for k, poison in enumerate((False, True, False)):
        w.grad = torch.randn(300, device=dev)
        if poison:
            w.grad[7] = float("inf")
        if k == 2:
            q.grad = torch.randn(50, device=dev)
        opt.step()
    ref = FusedAdamW([alone], lr=LR, weight_decay=WD, max_grad_norm=1e9)
    alone.grad = q.grad.clone()
    ref.step()
    assert opt.skipped_steps() == 1 and int(opt.state[q]["step"]) == 2 and int(opt.state[w]["step"]) == 3
    assert torch.equal(q.data, alone.data) and torch.equal(opt.state[q]["exp_avg"], ref.state[alone]["exp_avg"])
    steps = [float(v["step"]) for v in opt.state_dict()["state"].values()]
    assert steps == [2.0, 1.0]


def test_step_reads_nothing_back(dev, monkeypatch):
    """`step()` with the guard on makes no .item() / .cpu() / synchronize call of its own."""
    opt, arena, loose = _optimizer(dev, max_grad_norm=1.0)
    _set_grads(arena, loose, _grad_values(5, 1.0))
    opt.step()                                                           # (state set-up)

    def forbidden(*a, **k):
        raise AssertionError("host read-back inside FusedAdamW.step()")
    _set_grads(arena, loose, _grad_values(6, 1.0))
    with monkeypatch.context() as mp_:
        for name in ("item", "cpu", "tolist", "numpy"):
            mp_.setattr(torch.Tensor, name, forbidden)
        mp_.setattr(torch.cuda, "synchronize", forbidden)
        opt.step()
    assert opt.grad_norm.tolist()[2] == 1.0


# ---- the whole model through ClassifierExperiment -------------------------------------------------------------------------------
def test_whole_model_clipped_training_follows_the_torch_path(dev, tmp_path):
    from tests.test_experiment_gpu import _delta_agreement, _experiment, _loader, _weights
    runs = {}
    for name, fused in (("fused", "true"), ("torch", "false")):
        exp = _experiment(str(tmp_path / name), [f"optimizer.config.fused={fused}", "optimizer.config.max_grad_norm=0.1",
                                                 "optimizer.config.learning_rate=5e-4"], _loader(steps=1))
        w0 = _weights(exp)
        exp.scheduler.step()                      # leave the reference's lr-0 first epoch
        exp.scheduler.step()
        exp.train()                               # one step
        if name == "fused":
            opt = exp.optimizer
            grads = [p.grad for p in exp.model.parameters() if p.grad is not None]
            ref = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
            got = opt.grad_norm.tolist()
            print(f"whole model: grad_norm {got[0]!r} fp64 {ref!r} coef {got[1]!r}")
            assert abs(got[0] - ref) <= 1e-6 * ref and got[2] == 1.0
            assert got[1] < 1.0                                          # the bound binds
            ia, ta = exp.model.image_encoder.arena, exp.model.text_encoder.arena
            assert id(ia) in opt._flat and id(ta) in opt._flat           # both arenas took the one-launch path ...
            loose = [p for p in exp.model.parameters() if p.grad is not None and getattr(p, "_mmg_arena", None) is None]
            assert opt._piece_sizes == (ia.size, ta.size) + tuple(p.numel() for p in loose)      # ... and went into the norm as one piece each
            assert int(opt.state[ia.params[0]]["step"]) == 1 and opt.skipped_steps() == 0
        else:
            assert type(exp.optimizer).__name__ == "AdamW" and exp.skipped_steps == 0 and float(exp._last_grad_norm) > 0.1
        exp.train_dataloader = _loader(steps=5, seed=6)
        exp.train()                               # five more
        runs[name] = (_weights(exp), w0)
    cos, ratio = _delta_agreement(runs["fused"][0], runs["torch"][0], runs["torch"][1])
    print(f"clipped fused vs clipped torch AdamW after 6 steps: movement cosine {cos:.4f}, norm ratio {ratio:.4f}")
    assert cos > 0.9 and 0.95 < ratio < 1.05, (cos, ratio)               # test_fused_adamw_built_before_first_forward_trains_the_towers' bars


# ---- two ranks on the one GPU -----------------------------------------------------------------------------------------------------
def _clip_worker(rank, world, port, tmp, q):
    for p in (ROOT, os.path.join(ROOT, "mmg-clip_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    try:
        from mmgclip import distributed
        from tests.test_experiment_gpu import _experiment, _HalfLoader, _loader, _weights
        comm = distributed.init_from_env("gloo")
        exp = _experiment(f"{tmp}/r{rank}", ["optimizer.config.fused=true", "optimizer.config.learning_rate=1e-3",
                                             "optimizer.config.max_grad_norm=0.1"], _HalfLoader(_loader(steps=2, n=8, seed=31), rank, world), comm=comm)
        w0 = _weights(exp)
        exp.scheduler.step()
        exp.train()                                # two clipped steps
        torch.cuda.synchronize()
        w1 = _weights(exp)
        moved = max(float((w1[k] - w0[k]).abs().max()) for k in w0)
        q.put((rank, "ok", (exp.optimizer.grad_norm.cpu().numpy().view(np.uint32).tolist(), exp.optimizer.skipped_steps(), moved,
                            {k: v.numpy() for k, v in w1.items()})))
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))


def test_two_ranks_clip_with_the_same_bits(dev, tmp_path):
    """The norm is taken after GradSync.finish() on the reduced gradients: both ranks compute the same norm and coefficient, bit for bit,
    and stay replicas of each other."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_clip_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted([q.get(timeout=420) for _ in range(2)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
    assert all(r[1] == "ok" for r in results), [r[2] for r in results if r[1] != "ok"]
    assert all(p.exitcode == 0 for p in procs)
    (bits0, sk0, moved0, sd0), (bits1, sk1, moved1, sd1) = results[0][2], results[1][2]
    assert bits0 == bits1 and sk0 == sk1 == 0, (bits0, bits1)
    norm, coef, finite = np.array(bits0[:3], dtype=np.uint32).view(np.float32).tolist()
    assert finite == 1.0 and norm > 0.1 and coef < 1.0                   # the clip was active
    assert moved0 > 1e-4
    for k in sd0:
        assert np.array_equal(sd0[k], sd1[k]), k
