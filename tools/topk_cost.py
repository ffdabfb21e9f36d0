#!/usr/bin/env python3
"""What the nearest-neighbour search costs at D = 512 on one device, for n queries against N gallery rows at
(n, N) = (256, 6441), (256, 16384), (16384, 16384) and k = 1, 5, 32:

  * the fused launch (`head._HipTopKBackend.topk`, one `mmg_topk_rows`);
  * the dense torch route on the same tensors (`X @ Y.T`, then `torch.topk`);
  * the peak of `torch.cuda.max_memory_allocated` above the inputs of both routes, results alive.  The fused route's claim - the two
    [n,k] lists and no [n,N] allocation - is asserted.

HIP events around single calls, the two arms alternating, median (min, max).  No ratio is promised: the table is what was measured.

    python tools/topk_cost.py [--reps 10] [--warmup 2] [--out profiles/topk.md]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import torch                                                                    # noqa: E402
from mmgclip import head                                                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--shapes", type=int, nargs="+", default=[256, 6441, 256, 16384, 16384, 16384], help="n N pairs")
ap.add_argument("--ks", type=int, nargs="+", default=[1, 5, 32])
ap.add_argument("--out", default=None)
args = ap.parse_args()
if len(args.shapes) % 2:
    sys.exit("--shapes takes n N pairs")
if not torch.cuda.is_available():
    sys.exit("topk_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")
ARCH = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
CUS = torch.cuda.get_device_properties(0).multi_processor_count
PART = f"MI355X ({ARCH}, {CUS} CUs)" if ARCH == "gfx950" else f"{torch.cuda.get_device_name(0)} ({ARCH})"
D = 512


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    del out
    return a.elapsed_time(b)


def peak_above_inputs(fn):
    """Peak of the allocator above what is live before the call, with the call's results still alive."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def fmt(ms):
    return f"{statistics.median(ms):.3f} ({min(ms):.3f}, {max(ms):.3f})"


time_rows, memory_rows, slower = [], [], []
for n, N in zip(args.shapes[::2], args.shapes[1::2]):
    g = torch.Generator().manual_seed(N + n)
    Y = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).to(dev)
    X = torch.nn.functional.normalize(Y[torch.randint(0, N, (n,), generator=g).to(dev)] +
                                      0.8 * torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=1).to(dev), dim=1).contiguous()
    for k in args.ks:
        variants = {"fused": lambda: head._HipTopKBackend.topk(X, Y, k), "dense": lambda: torch.topk(X @ Y.t(), k, dim=1)}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in variants}
        order = list(variants)
        for rep in range(args.reps):
            for name in (order if rep % 2 == 0 else order[::-1]):
                t[name].append(event_ms(variants[name]))
        mem = {name: peak_above_inputs(fn) for name, fn in variants.items()}
        claim = n * k * 8                                          # the two [n,k] lists, 4 bytes an entry
        assert mem["fused"] <= claim + 2 * 512, (mem, claim)      # (the allocator rounds each of the two blocks up to 512 bytes)
        (fs, fj), dn = variants["fused"](), variants["dense"]()
        same = float((fj.long() == dn.indices).all(dim=1).double().mean())
        med = {name: statistics.median(v) for name, v in t.items()}
        flop = 2.0 * n * N * D
        time_rows.append(f"| {n} | {N} | {k} | {(n + 31) // 32} | {fmt(t['fused'])} | {flop / med['fused'] / 1e9:.1f} | {fmt(t['dense'])} | "
                         f"{med['dense'] / med['fused']:.2f}x | {same:.4f} |")
        memory_rows.append(f"| {n} | {N} | {k} | {mem['fused']} | {claim} | {mem['dense']} ({mem['dense'] / 2 ** 20:.1f} MiB) | {n * N * 4} |")
        if med["fused"] > med["dense"]:
            slower.append(f"n = {n}, N = {N}, k = {k}: fused {med['fused']:.3f} ms, dense {med['dense']:.3f} ms")
    del X, Y
    torch.cuda.empty_cache()

lines = [
    "# Nearest-report search: the fused top-K launch against the dense route",
    "",
    f"{PART}, torch {torch.__version__}; `tools/topk_cost.py`: D = {D}, n queries against N gallery rows, no exclusion, one process.  HIP "
    f"events around single calls, {args.warmup} warm-up and {args.reps} timed calls of each arm, the order alternating; ms, median (min, "
    "max).  `fused` is one `mmg_topk_rows` launch of `ceil(n / 32)` workgroups (the column `workgroups`: the device has "
    f"{CUS} CUs, so a launch of 8 workgroups leaves most of it idle); TFLOP/s counts `2 n N D` FLOP over the whole call and is a "
    "whole-call rate, not a share of peak.  `dense` is `X @ Y.T` followed by `torch.topk(k)` on the same tensors.  `same rows` is the "
    "share of queries to which the two routes give the same k indices in the same order; they form the dot products in different orders "
    "and `torch.topk` promises no tie order, so on random unit rows they may differ where two scores are within rounding (the tests compare "
    "the kernel with float64 intervals instead).",
    "",
    "| n | N | k | workgroups | fused | TFLOP/s | dense | dense / fused | same rows |",
    "|---|---|---|---|---|---|---|---|---|",
] + time_rows + [
    "",
    ("The fused launch is SLOWER than the dense route at: " + "; ".join(slower) + "." if slower else
     "The fused launch was not slower than the dense route at any shape measured."),
    "",
    "## Memory",
    "",
    "Peak of `torch.cuda.max_memory_allocated` above the inputs, results alive, bytes.  The claim that can be derived - the two `[n,k]` "
    "lists and no `[n,N]` allocation - is asserted by the tool (`fused` at most the claim plus the allocator's rounding of two blocks).",
    "",
    "| n | N | k | fused peak | claim (n k 8) | dense peak | one fp32 [n,N] |",
    "|---|---|---|---|---|---|---|",
] + memory_rows
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
