#!/usr/bin/env python3
"""Sigmoid pairwise loss, head only: `head.fused_sigmoid_loss` with positives = diagonal and positives = clusters (the latter adds the
text similarity, the clustering kernel and its 4-byte read-back of the cluster count) against `head.fused_clip_loss`, the softmax loss
every shipped config trains with.  Three different losses are timed, not three ways to one number: the point is what choosing the
sigmoid loss costs in the head, which is well under 1 % of a training step either way.

Forward and forward + backward from the L2-normalised embeddings, HIP events around single calls, the three variants alternating,
median (min, max).  Shapes: N = 256, D = 512 (the product batch) and N = 2048, D = 512; one process (`comm=None`); the text side falls
into N / 4 clusters at the threshold.

    python tools/sigmoid_loss_cost.py [--reps 20] [--warmup 3] [--out profiles/sigmoid_loss.md]
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
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("sigmoid_loss_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")
ARCH = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
PART = (f"MI355X ({ARCH}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)" if ARCH == "gfx950"
        else f"{torch.cuda.get_device_name(0)} ({ARCH})")
THRESHOLD = 0.65


def inputs(N, D, k, seed=0):
    """Normalised image / text embeddings whose text side falls into exactly k clusters at the threshold."""
    g = torch.Generator().manual_seed(seed)
    protos = torch.nn.functional.normalize(torch.randn(k, D, generator=g), dim=1)
    member = (torch.arange(N) % k)[torch.randperm(N, generator=g)]
    txt = torch.nn.functional.normalize(protos[member] + 0.4 / D ** 0.5 * torch.randn(N, D, generator=g), dim=1)
    img = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
    return img.to(dev), txt.to(dev)


def timed(step):
    """(forward ms, forward + backward ms) of one call of `step`, which returns the loss."""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    loss = step()
    e[1].record()
    loss.backward()
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[0].elapsed_time(e[2])


def fmt(ms):
    return f"{statistics.median(ms):.3f} ({min(ms):.3f}, {max(ms):.3f})"


rows = []
for N, D in ((256, 512), (2048, 512)):
    k = N // 4
    img, txt = inputs(N, D, k)
    a, b = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
    s = torch.tensor(10.0, device=dev, requires_grad=True)
    bias = torch.tensor(-10.0, device=dev, requires_grad=True)
    variants = {
        "clip": lambda: head.fused_clip_loss(a, b, s),
        "sigmoid, diagonal": lambda: head.fused_sigmoid_loss(a, b, s, bias, "diagonal", THRESHOLD)[0],
        "sigmoid, clusters": lambda: head.fused_sigmoid_loss(a, b, s, bias, "clusters", THRESHOLD)[0],
    }
    for fn in variants.values():
        for _ in range(args.warmup):
            a.grad = b.grad = s.grad = bias.grad = None
            loss = fn()
            loss.backward()
        assert torch.isfinite(loss).item()
    k_seen = int(head.fused_sigmoid_loss(a, b, s, bias, "clusters", THRESHOLD)[1].max().item()) + 1
    assert k_seen == k, (k_seen, k)
    t = {name: ([], []) for name in variants}
    order = list(variants)
    for rep in range(args.reps):
        for name in (order if rep % 2 == 0 else order[::-1]):                  # alternating order
            a.grad = b.grad = s.grad = bias.grad = None
            f, fb = timed(variants[name])
            t[name][0].append(f)
            t[name][1].append(fb)
    base = statistics.median(t["clip"][1])
    for name in order:
        rows.append(f"| {N} | {D} | {name} | {fmt(t[name][0])} | {fmt(t[name][1])} | {statistics.median(t[name][1]) / base:.2f}x |")

lines = [
    "# Sigmoid pairwise loss, head only: against the fused softmax CLIP loss",
    "",
    f"{PART}, torch {torch.__version__}; `tools/sigmoid_loss_cost.py`: from the L2-normalised embeddings to the loss (forward) and on to "
    f"dI, dT, dscale (and dbias) (forward + backward), one process (`comm=None`).  HIP events around single calls, {args.warmup} warm-up and "
    f"{args.reps} timed calls of each variant, the order alternating; ms, median (min, max).  `clusters` adds the [N,N] text similarity, the "
    "clustering kernel and the read-back of the cluster count (4 bytes, one synchronisation); the text falls into N / 4 clusters.  The last "
    "column is forward + backward over the CLIP loss's.  Not measured: more than one rank (the sigmoid loss then saves the second exchange, "
    "the all-gather of the two log-sum-exp vectors).",
    "",
    "| N | D | loss | forward | fwd + bwd | / clip |",
    "|---|---|---|---|---|---|",
] + rows
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
