"""The error bars of tests/attention_ref.py, checked without a GPU on every row of the table the GPU tests run (attention_ref.CASES):
an emulation of the kernels' arithmetic (float64 with their two bf16 rounding points) stays inside every bar, and every mutation of it
(a dropped key, exchanged V rows, a shifted mask, a dS tile without its scale or 2 % off, a missing delta, an unwritten 16-row block, an lse off
by 1e-3) leaves at least one.  This is how the GPU tests are known to fail for a subtly wrong kernel."""
import pytest
import torch

from tests import attention_ref as R


def _head0(d):
    """Sequence 0, head 0 of a dict of [B, heads, ...] / [B, S] tensors (the mutations act there)."""
    return {k: (None if t is None else t[0:1, 0:1] if t.dim() >= 3 else t[0:1]) for k, t in d.items()}


def _worst(res):
    return max(w for w, _ in res.values())


@pytest.fixture(scope="module")
def mutation_ratios():
    """{mutation: {case id: worst ratio over the outputs}}; also the unmutated emulation's as mutation None."""
    out = {m: {} for m in (None,) + R.MUTATIONS}
    for case in R.CASES:
        inp, ref, A = R.prepared(case)
        out[None][case.id] = _worst(R.check_all(case, inp, ref, A, R.emulate(case, inp, ref)))
        i0, r0, a0 = _head0(inp), _head0(ref), _head0(A)
        for m in R.MUTATIONS:
            out[m][case.id] = _worst(R.check_all(case, i0, r0, a0, R.emulate(case, i0, r0, m)))
    return out


def test_case_ids_are_unique_and_every_instantiation_gets_flat_peaked_and_readout():
    assert len({c.id for c in R.CASES}) == len(R.CASES)
    seen = {}
    for c in R.CASES:
        for inst in R.instantiations(c):
            seen.setdefault(inst, set()).add(c.regime)
    want = {("fwd", nt, d) for nt in (6, 8, 16, 32) for d in (False, True)} | {("bwd", False), ("bwd", True)}
    want |= {("flash_fwd", rb, m) for rb in (1, 2, 4) for m in (False, True)}
    want |= {("flash_dq", rb, m, False) for rb in (1, 2, 4) for m in (False, True)}
    want |= {("flash_dkv", rb, m, False) for rb in (1, 2, 3) for m in (False, True)}
    want |= {(k, 2, m, True) for k in ("flash_dq", "flash_dkv") for m in (False, True)}
    assert want <= set(seen), want - set(seen)
    for inst in want:
        assert {"flat", "peaked", "readout"} <= seen[inst], (inst, seen[inst])
    for rb in (1, 2, 4):
        assert {"offset", "ascending", "descending"} & (seen[("flash_fwd", rb, False)] | seen[("flash_fwd", rb, True)])
    tiled_fwd = set().union(*(seen[("flash_fwd", rb, m)] for rb in (1, 2, 4) for m in (False, True)))
    assert {"offset", "ascending", "descending"} <= tiled_fwd


def test_masks_leave_an_attended_key_and_left_padding_covers_a_whole_tile():
    for c in R.CASES:
        v = R.make_valid(c)
        assert v.any(-1).all(), c.id
        if c.family == "tiled" and c.mask == "left" and c.S > 64:
            assert not v[:, :64].any(), c.id


def test_the_emulation_stays_inside_every_bar(mutation_ratios):
    worst = mutation_ratios[None]
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def test_every_mutation_leaves_a_bar(mutation_ratios):
    by_id = {c.id: c for c in R.CASES}

    def has_ds(c):
        """A dS tile exists where there is a backward and sequence 0 attends more than one key (the softmax of a single key is the
        constant 1, whose dS is identically zero)."""
        return c.has_bwd and int(R.make_valid(c)[0].sum()) > 1

    for m in R.MUTATIONS:
        ratios = mutation_ratios[m]
        assert max(ratios.values()) > 1.0, (m, max(ratios.values()))
        if m == "ds_tile_2pct":                  # the smallest mutation: caught in every flat case that has a dS tile
            missed = {k: v for k, v in ratios.items() if not v > 1.0 and by_id[k].regime == "flat" and has_ds(by_id[k])}
            assert not missed, (m, missed)
        if m in R.TILE_LOCAL:                    # local to one tile: caught wherever that tile exists
            missed = {k: v for k, v in ratios.items() if not v > 1.0 and (not m.startswith("ds_tile") or has_ds(by_id[k]))}
            assert not missed, (m, missed)


def test_the_lse_bar_is_four_times_tighter_than_the_old_kernel_to_kernel_comparison():
    """At the magnitudes of test_attention_long_fwd_bwd (unit normal q, k; scale 1/8) the bar must be <= 1e-4 / 4."""
    for case in R.CASES:
        if case.regime == "flat" and case.scale == 0.125:
            inp, ref, A = R.prepared(case)
            assert A["lse"][inp["rows"][:, None, :].expand_as(A["lse"])].max().item() <= 2.5e-5, case.id


def test_reference_gradients_are_the_autograd_gradients():
    """The closed forms of the reference (dV, dS, dQ, dK with dropout) against torch autograd in float64."""
    case = next(c for c in R.CASES if c.family == "drop" and c.S == 97 and c.regime == "flat")
    inp, ref, _ = R.prepared(case)
    q, k, v = [inp[n].clone().requires_grad_(True) for n in "qkv"]
    s = (q @ k.transpose(-1, -2)) * case.scale
    s = s.masked_fill(~inp["valid"][:, None, None, :], float("-inf"))
    ctx = (s.softmax(-1) * inp["keep"].to(R.F64) * R._drop_scale(case.p)) @ v
    (ctx * inp["dO"]).sum().backward()
    for name, t in (("dQ", q), ("dK", k), ("dV", v)):
        assert torch.allclose(ref[name], t.grad, rtol=1e-10, atol=1e-12), name
    assert torch.allclose(ref["ctx"], ctx.detach(), rtol=1e-12, atol=1e-14)
    assert torch.allclose(ref["lse"], torch.logsumexp(s, -1).detach(), rtol=1e-12, atol=1e-12)
