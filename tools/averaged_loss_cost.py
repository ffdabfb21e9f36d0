#!/usr/bin/env python3
"""AveragedMedicalCLIPLoss, head only: the fused path (`head.fused_averaged_loss`: similarity + clustering, centroids, two labelled
rows forwards, four labelled rows backwards; no [n,N] logits) against the dense path (two materialised [n,n] logit matrices with
autograd, similarity + clustering, `ClusterMeanCols`, two dense cross-entropies, `mmg_clip_rows_bwd_dense` twice).  The dense path is
the one every earlier commit has: this tool times it as it stands in the tree it is run from.

Forward and forward + backward from the L2-normalised embeddings, HIP events around single calls, the two paths alternating, median
(min, max).  Both paths include the 4-byte read-back of the cluster count.  Shapes: n = 256, D = 512 (the product batch) and
N = 2048, D = 512, each with k in {16, N/4, N} clusters.

    python tools/averaged_loss_cost.py [--reps 20] [--warmup 3] [--out profiles/averaged_loss_cost.md]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import torch                                                                    # noqa: E402
from mmgclip import head                                                        # noqa: E402
from mmgclip.loss.losses import AveragedMedicalCLIPLoss                         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("averaged_loss_cost.py measures on the GPU: no device found, nothing measured")
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
for N, D, ks in ((256, 512, (16, 64, 256)), (2048, 512, (16, 512, 2048))):
    for k in ks:
        img, txt = inputs(N, D, k)
        a, b = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
        s = torch.tensor(14.2857, device=dev, requires_grad=True)
        dense_crit, fused_crit = AveragedMedicalCLIPLoss(THRESHOLD), AveragedMedicalCLIPLoss(THRESHOLD, fused=True)

        def dense():
            li, lt = head.ScaledLogits.apply(a, b, s)
            return dense_crit(image_embeddings=a, text_embeddings=b, logit_scale=s, logits_per_image=li, logits_per_text=lt)[0]

        def fused():
            return fused_crit(image_embeddings=a, text_embeddings=b, logit_scale=s)[0]

        variants = {"dense": dense, "fused": fused}
        losses = {}
        for name, fn in variants.items():
            for _ in range(args.warmup):
                a.grad = b.grad = s.grad = None
                loss = fn()
                loss.backward()
            losses[name] = loss.item()
        k_seen = int(fused_crit(image_embeddings=a, text_embeddings=b, logit_scale=s)[1].max().item()) + 1
        assert k_seen == k, (k_seen, k)
        assert abs(losses["dense"] - losses["fused"]) <= 1e-5 * abs(losses["dense"]), losses        # the same quantity is being timed
        t = {name: ([], []) for name in variants}
        for _ in range(args.reps):
            for name, fn in variants.items():
                a.grad = b.grad = s.grad = None
                f, fb = timed(fn)
                t[name][0].append(f)
                t[name][1].append(fb)
        med = {name: statistics.median(t[name][1]) for name in variants}
        rows.append(f"| {N} | {D} | {k} | {fmt(t['dense'][0])} | {fmt(t['fused'][0])} | {fmt(t['dense'][1])} | {fmt(t['fused'][1])} | "
                    f"{med['dense'] / med['fused']:.2f}x |")

lines = [
    "# AveragedMedicalCLIPLoss, head only: fused path against the dense path",
    "",
    f"{PART}, torch {torch.__version__}; `tools/averaged_loss_cost.py`: from the L2-normalised embeddings to the loss (forward) and on to "
    f"dI, dT, dscale (forward + backward), one process (`comm=None`).  HIP events around single calls, {args.warmup} warm-up and {args.reps} "
    "timed calls of each path, the paths alternating; ms, median (min, max).  Both paths compute the [N,N] text similarity, run the "
    "clustering kernel and read the cluster count back (4 bytes, one synchronisation).  The dense path is unchanged from the earlier "
    "commits.  The last column is dense / fused of the forward + backward medians.",
    "",
    "| N | D | k | forward, dense | forward, fused | fwd + bwd, dense | fwd + bwd, fused | dense / fused |",
    "|---|---|---|---|---|---|---|---|",
] + rows
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
