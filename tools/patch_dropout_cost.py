#!/usr/bin/env python3
"""What patch dropout saves: forward + backward of the ViT-B/16 image tower alone, in one process on one box, at several rates.
Under train() an image keeps K = max(1, int(P * (1 - rate))) patches plus the class token (mmgclip/patch_dropout.py) and every layer runs on
S_eff = 1 + K tokens, so the step should shorten as the FLOP model says - the GEMMs in proportion to S, the attention to S^2 - minus what the
draw, the row gather and the smaller launches cost.

  C4's image side:  ViT-B/16, 1024 x 1024 (P = 4096, S = 4097), micro-batches of 16, rates 0 / 0.25 / 0.5 / 0.75

HIP events around windows of `reps` steps; the rates alternate, `rounds` windows each, one untimed step after every change of rate.  Every
step draws a fresh seed from the tower's own stream.  Rate 0 runs the launches of a tower without the argument: it is the yardstick.  Peak
memory is torch's max_memory_allocated over a window.  The index launch (mmg_patch_keep_indices for the whole batch) is timed apart.

    python tools/patch_dropout_cost.py [--batch 64] [--size 1024] [--micro-batch 16] [--reps 2] [--rounds 3] [--out profiles/patch_dropout.md]
"""
import argparse
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import torch                                                                    # noqa: E402
from mmgclip import patch_dropout as PD                                         # noqa: E402
from mmgclip._hip import call, ptr, stream                                      # noqa: E402
from mmgclip.networks.encoder import ViTB16Encoder                              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--micro-batch", type=int, default=16)
ap.add_argument("--layers", type=int, default=12)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("patch_dropout_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")
RATES = (0.0, 0.25, 0.5, 0.75)
HID = 768


def flop_model(S):
    """Forward FLOPs of one layer per image, up to a common factor: GEMMs 24 S H^2 (qkv 6, out 2, MLP 16), attention 4 S^2 H."""
    return 24.0 * S * HID * HID + 4.0 * S * S * HID


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


torch.manual_seed(0)
tower = ViTB16Encoder(image_size=args.size, layers=args.layers, micro_batch=args.micro_batch).to(dev).train()
P = tower.seq - 1
pix = torch.rand(args.batch, 1, args.size, args.size, generator=torch.Generator().manual_seed(1)).to(dev)
wgt = torch.randn(args.batch, HID, device=dev)


def step():
    tower.zero_grad(set_to_none=True)
    (tower(pix) * wgt).sum().backward()


ms = {r: [] for r in RATES}
peak = {r: 0 for r in RATES}
for _ in range(args.rounds):
    for r in RATES:
        tower.patch_dropout = r
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms[r].append(timed(step, args.reps))
        peak[r] = max(peak[r], torch.cuda.max_memory_allocated())

draw = {}
for r in RATES[1:]:
    K = PD.keep_count(P, r)
    keep = torch.empty(args.batch, K, device=dev, dtype=torch.int32)
    slot = torch.empty(args.batch, P, device=dev, dtype=torch.int32)
    seeds = iter(range(1, 1000))
    launch = lambda: call("mmg_patch_keep_indices", next(seeds), None, args.batch, P, K, ptr(keep), ptr(slot), stream())  # noqa: E731
    timed(launch, 3)
    draw[r] = [timed(launch, 20) for _ in range(args.rounds)]


def fmt(v, unit="ms", d=1):
    return f"{statistics.median(v):.{d}f} {unit} (min {min(v):.{d}f}, max {max(v):.{d}f}, {len(v)} windows)"


base = statistics.median(ms[0.0])
lines = [
    "# Patch dropout: what running the ViT tower on the kept tokens saves",
    "",
    f"Box `{socket.gethostname()}`, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; `tools/patch_dropout_cost.py`: ViT-B/16 image tower alone "
    f"({args.layers} layers), forward + backward, {args.batch} images of {args.size} x {args.size} (P = {P} patches) in micro-batches of "
    f"{args.micro_batch}, bf16.  HIP events, windows of {args.reps} steps, rates alternating in one process, median (min, max) of {args.rounds} "
    "windows each; a fresh seed every step.  Rate 0 executes the launches of a tower built without the argument.  FLOP model: per layer "
    "24 S H^2 for the GEMMs plus 4 S^2 H for the attention, relative to the full sequence.",
    "",
    "| rate | K | S_eff | forward + backward | against rate 0 | FLOP model | peak memory | index launch (whole batch) |",
    "|---|---|---|---|---|---|---|---|",
]
for r in RATES:
    K = PD.keep_count(P, r) if r > 0 else P
    lines.append(f"| {r} | {K} | {1 + K} | {fmt(ms[r])} | {statistics.median(ms[r]) / base:.3f} | {flop_model(1 + K) / flop_model(1 + P):.3f} | "
                 f"{peak[r] / 2 ** 30:.2f} GiB | {fmt(draw[r], 'ms', 3) if r > 0 else 'none'} |")
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
