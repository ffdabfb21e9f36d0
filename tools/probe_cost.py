#!/usr/bin/env python3
"""What the linear probe costs on one device at D = 512 and D = 768 with C = 2 and C = 6 classes, n rows:

  * one evaluation of (L, dW, db): the fused route (`head._HipProbeBackend.evaluate`: `mmg_probe_rows`, two launches, one read of X)
    against the dense torch route on the same tensors (`LinearProbe.dense_evaluate`: two reads of X, two [n,C] temporaries).  A call
    takes a fraction of a millisecond, so one HIP event pair brackets a BATCH of back-to-back calls (`--batch`, 50) and the figure is
    the batch's time over its calls; the two arms alternate, median (min, max) over the batches;
  * a whole fit (`LinearProbe.fit`, the same l2, max_iter and gtol) by both routes, and sklearn `LogisticRegression(lbfgs)` on the
    host on the same rows with C = 1 / (l2 S) and the same iteration cap.  Wall clock around the call with the device synchronised:
    a fit is host-driven (one upload of W, b and one read-back per evaluation), so the host's share belongs in the figure;
  * the peak of `torch.cuda.max_memory_allocated` above the inputs of one evaluation, result alive.

No ratio is promised: the table is what was measured, including where the fused route loses.

    python tools/probe_cost.py [--n 32768 2048] [--reps 20] [--batch 50] [--warmup 5] [--out profiles/linear_probe.md] [--commit TEXT]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import torch                                                                    # noqa: E402
from mmgclip import head, probe                                                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[32768, 2048])
ap.add_argument("--reps", type=int, default=20, help="timed batches per arm")
ap.add_argument("--batch", type=int, default=50, help="back-to-back calls inside one event pair")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--fit-reps", type=int, default=3)
ap.add_argument("--max-iter", type=int, default=100)
ap.add_argument("--l2", type=float, default=1e-3)
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default=None, help="what the table says it was taken at (default: git rev-parse HEAD)")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("probe_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")
ARCH = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
CUS = torch.cuda.get_device_properties(0).multi_processor_count
PART = f"MI355X ({ARCH}, {CUS} CUs)" if ARCH == "gfx950" else f"{torch.cuda.get_device_name(0)} ({ARCH})"
commit = args.commit
if commit is None:
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown (no git checkout)"


def event_ms(fn, calls):
    """ms per call of `calls` back-to-back calls between one pair of events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_above_inputs(fn):
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


def problem(n, D, C, seed=0):
    """Overlapping Gaussian blobs: a fit that takes a few dozen iterations."""
    g = torch.Generator().manual_seed(seed + n + D + C)
    centres = torch.randn(C, D, generator=g) * (2.0 / D ** 0.5)
    y = torch.arange(n) % C
    return (centres[y] + torch.randn(n, D, generator=g)).contiguous(), y.contiguous()


eval_rows, fit_rows, memory_rows, slower = [], [], [], []
for n in args.n:
    for D in (512, 768):
        for C in (2, 6):
            Xh, yh = problem(n, D, C)
            X, y = Xh.to(dev), yh.to(dev)
            g = torch.Generator().manual_seed(1)
            W, b = (torch.randn(C, D, generator=g) * 0.05).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
            variants = {"fused": lambda: head._HipProbeBackend.evaluate(X, W, b, y), "dense": lambda: probe.LinearProbe.dense_evaluate(X, W, b, y)}
            for fn in variants.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            t = {name: [] for name in variants}
            order = list(variants)
            for rep in range(args.reps):
                for name in (order if rep % 2 == 0 else order[::-1]):
                    t[name].append(event_ms(variants[name], args.batch))
            mem = {name: peak_above_inputs(fn) for name, fn in variants.items()}
            med = {name: statistics.median(v) for name, v in t.items()}
            groups = min((n + 31) // 32, CUS)
            gbs = n * D * 4 / med["fused"] / 1e6
            diff = float((variants["fused"]() - variants["dense"]()).abs().max() / variants["dense"]().abs().max())
            eval_rows.append(f"| {n} | {D} | {C} | {groups} | {fmt(t['fused'])} | {gbs:.0f} | {fmt(t['dense'])} | {med['dense'] / med['fused']:.2f}x | {diff:.1e} |")
            memory_rows.append(f"| {n} | {D} | {C} | {mem['fused']} | {mem['dense']} ({mem['dense'] / 2 ** 20:.2f} MiB) | {2 * n * C * 4} |")
            if med["fused"] > med["dense"]:
                slower.append(f"one evaluation at n = {n}, D = {D}, C = {C}: fused {med['fused']:.3f} ms, dense {med['dense']:.3f} ms")
            # whole fits
            fits = {}
            for name, fused in (("fused", True), ("dense", False)):
                runs = []
                for _ in range(args.fit_reps):
                    ms, lp = wall_ms(lambda: probe.LinearProbe(l2=args.l2, max_iter=args.max_iter, gtol=1e-4, fused=fused).fit(X, y, n_classes=C))
                    runs.append(ms)
                fits[name] = (runs, lp)
            from sklearn.linear_model import LogisticRegression
            Xn, yn = Xh.numpy(), yh.numpy()
            runs = []
            for _ in range(args.fit_reps):
                t0 = time.perf_counter()
                sk = LogisticRegression(C=1.0 / (args.l2 * n), max_iter=args.max_iter, tol=1e-4, solver="lbfgs").fit(Xn, yn)
                runs.append((time.perf_counter() - t0) * 1e3)
            f, d = fits["fused"], fits["dense"]
            acc = float((f[1].predict(X) == y).double().mean())
            acc_sk = float((sk.predict(Xn) == yn).mean())
            fit_rows.append(f"| {n} | {D} | {C} | {fmt(f[0])} | {f[1].n_iter_} / {f[1].n_evaluations_} | {fmt(d[0])} | {d[1].n_iter_} / {d[1].n_evaluations_} | "
                            f"{fmt(runs)} | {int(max(sk.n_iter_))} | {acc:.4f} / {acc_sk:.4f} |")
            if statistics.median(f[0]) > statistics.median(d[0]):
                slower.append(f"a whole fit at n = {n}, D = {D}, C = {C}: fused {statistics.median(f[0]):.1f} ms, dense {statistics.median(d[0]):.1f} ms")
            del X, y, W, b
            torch.cuda.empty_cache()

lines = [
    "# Linear probe: the fused one-pass evaluation against the dense route and sklearn",
    "",
    f"{PART}, torch {torch.__version__}; `tools/probe_cost.py` at {commit}; one process.  Rows are overlapping Gaussian blobs, labels "
    "`i mod C`, no class weights.",
    "",
    "## One evaluation of (L, dW, db)",
    "",
    f"One HIP event pair around a batch of {args.batch} back-to-back calls, {args.warmup} warm-up calls and {args.reps} timed batches of each "
    "arm, the order alternating; ms per call (the batch's time over its calls), median (min, max) over the batches.  `fused` is `mmg_probe_rows`: `workgroups` persistent workgroups (one per CU, never more than `ceil(n / 32)`) and the small "
    "finalising launch; GB/s is `4 n D` bytes, the one read of X, over the whole call - a whole-call rate, not a share of peak.  `dense` "
    "is `LinearProbe.dense_evaluate` on the same tensors.  `rel diff` is the largest difference of the two results over the largest entry.",
    "",
    "| n | D | C | workgroups | fused | GB/s | dense | dense / fused | rel diff |",
    "|---|---|---|---|---|---|---|---|---|",
] + eval_rows + [
    "",
    "## A whole fit",
    "",
    f"`LinearProbe(l2={args.l2}, max_iter={args.max_iter}, gtol=1e-4).fit`, wall clock with the device synchronised, {args.fit_reps} runs, ms, "
    "median (min, max); `it / ev` = L-BFGS iterations / evaluations.  Every evaluation uploads W, b and reads the fp64 result back, so a "
    f"fit's time is mostly the host's round trips at these sizes.  `sklearn` is `LogisticRegression(C=1/(l2 n), solver='lbfgs', "
    f"max_iter={args.max_iter}, tol=1e-4)` on the host on the same fp32 rows (for C = 2 it fits the binary model, half the unknowns).  "
    "`accuracy` is on the training rows, ours / sklearn's.",
    "",
    "| n | D | C | fused fit | it / ev | dense fit | it / ev | sklearn fit | sklearn it | accuracy |",
    "|---|---|---|---|---|---|---|---|---|---|",
] + fit_rows + [
    "",
    ("The fused route is SLOWER than the dense route at: " + "; ".join(slower) + "." if slower else
     "The fused route was not slower than the dense route at any shape measured."),
    "",
    "## Memory",
    "",
    "Peak of `torch.cuda.max_memory_allocated` above the inputs of one evaluation, result alive, bytes.  The fused route holds the "
    "workgroups' partials and the fp64 result; the dense route the logits, the softmax and what torch allocates around them.",
    "",
    "| n | D | C | fused peak | dense peak | two fp32 [n,C] |",
    "|---|---|---|---|---|---|",
] + memory_rows
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
