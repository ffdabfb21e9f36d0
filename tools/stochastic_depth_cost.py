#!/usr/bin/env python3
"""What stochastic depth saves: forward + backward of the ConvNeXt image tower alone, in one process on one box, at several rates.
Dropped samples are never computed (mmgclip/networks/convnext_sd.py), so the step should shorten by about the mean drop rate of the blocks,
minus what the image moves (csrc/stochastic_depth.hip) and the smaller launches cost.

  C2's image side:    ConvNeXt-T, 256 images of 1024 x 1024 in one micro-batch, rates 0 / 0.1 / 0.5
  base + checkpoint:  ConvNeXt-B, 256 images in checkpointed micro-batches of 64, rates 0 / 0.5

HIP events around windows of `reps` steps; the rates alternate, `rounds` windows each, one untimed step after every change of rate (the
working copies that bake the layer scale in are rebuilt then).  Every step draws a fresh seed from the tower's own stream.  Per block the
fraction of images kept, averaged over the timed steps, is printed beside 1 - p_b.

    python tools/stochastic_depth_cost.py [--batch 256] [--size 1024] [--reps 3] [--rounds 3] [--out profiles/r07_stochastic_depth.md]
"""
import argparse
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import numpy as np                                                              # noqa: E402
import torch                                                                    # noqa: E402
from mmgclip.networks import convnext_sd as SD                                  # noqa: E402
from mmgclip.networks.encoder import ConvNextBaseEncoder, ConvNextTinyEncoder   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stochastic_depth_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")

kept = []                                   # per scheduled micro-batch: the fraction of its images each block keeps
_schedule = SD.schedule


def _spy(keep):
    kept.append(np.asarray(keep).mean(1))
    return _schedule(keep)


SD.schedule = _spy                          # (convnext.py calls it through the module)


def measure(make, rates):
    """-> {rate: ([ms per step, one per window], kept fraction per block or None)}"""
    torch.manual_seed(0)
    tower = make().to(dev).train()
    with torch.no_grad():                   # make the blocks matter (layer scale is 1e-6 at init)
        for n, p in tower.named_parameters():
            if n.endswith("layer_scale"):
                p.fill_(0.5)
    tower.reseed_stochastic_depth(0)
    pix = torch.rand(args.batch, 1, args.size, args.size, generator=torch.Generator().manual_seed(1)).to(dev)
    wgt = torch.randn(args.batch, tower.model_output_dimension, device=dev)

    def step():
        tower.zero_grad(set_to_none=True)
        (tower(pix) * wgt).sum().backward()
    out = {r: ([], []) for r in rates}
    for _ in range(args.rounds):
        for r in rates:
            tower.stochastic_depth_prob = SD.check_rate(r)
            step()
            torch.cuda.synchronize()
            del kept[:]
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.reps):
                step()
            e.record()
            torch.cuda.synchronize()
            out[r][0].append(s.elapsed_time(e) / args.reps)
            out[r][1].extend(kept)
    return {r: (ms, np.mean(k, 0) if k else None) for r, (ms, k) in out.items()}, tower.depths


def fmt(ms):
    return f"{statistics.median(ms):.1f} ms (min {min(ms):.1f}, max {max(ms):.1f}, {len(ms)} windows)"


CASES = [
    ("ConvNeXt-T, one micro-batch (C2's image side)", lambda: ConvNextTinyEncoder(micro_batch=args.batch), (0.0, 0.1, 0.5)),
    ("ConvNeXt-B, checkpointed micro-batches of 64", lambda: ConvNextBaseEncoder(micro_batch=64, checkpoint=True), (0.0, 0.5)),
]
lines = [
    "# Stochastic depth: what skipping the dropped samples saves",
    "",
    f"Box `{socket.gethostname()}`, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; `tools/stochastic_depth_cost.py`: image tower alone, "
    f"forward + backward, {args.batch} images of {args.size} x {args.size}, bf16.  HIP events, windows of {args.reps} steps, rates alternating, "
    f"median (min, max) of {args.rounds} windows each; a fresh seed every step.  Ideal = 1 - mean(p_b) with every block weighted alike "
    "(a CNBlock costs the same FLOPs in every stage).",
    "",
    "| tower | rate | forward + backward | against rate 0 | ideal |",
    "|---|---|---|---|---|",
]
detail = []
for name, make, rates in CASES:
    res, depths = measure(make, rates)
    base = statistics.median(res[0.0][0])
    for r in rates:
        ms, frac = res[r]
        ideal = 1.0 - float(np.mean(SD.block_rates(r, depths)))
        lines.append(f"| {name} | {r} | {fmt(ms)} | {statistics.median(ms) / base:.3f} | {ideal:.3f} |")
        if frac is not None:
            detail += ["", f"{name}, rate {r}: images kept per block (measured over the timed steps | 1 - p_b)", ""]
            detail += ["| block | " + " | ".join(str(b) for b in range(len(frac))) + " |", "|---" * (len(frac) + 1) + "|",
                       "| kept | " + " | ".join(f"{v:.2f}" for v in frac) + " |",
                       "| 1 - p_b | " + " | ".join(f"{1 - p:.2f}" for p in SD.block_rates(r, depths)) + " |"]
    torch.cuda.empty_cache()
text = "\n".join(lines + detail) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
