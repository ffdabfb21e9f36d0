#!/usr/bin/env python3
"""What the foreground prior of patch dropout costs and what it keeps: the ViT-B/16 image tower alone, in one process on one box.
Under patch_prior = "foreground" an image keeps its K patches tissue first (mmgclip/patch_dropout.py): two more launches per forward -
`mmg_patch_foreground` (reads every pixel once, writes one count per patch) and `mmg_patch_keep_indices_prior` (the draw with the class bit
in front of its key) - and from there on the launches of the uniform prior at the same K.

  C4's image side:  ViT-B/16, 1024 x 1024 (P = 4096), 64 images in micro-batches of 16, rates 0.25 / 0.5 / 0.75, both priors

The images are SYNTHETIC, from a generator of this tool's own: a half-ellipse of noise (a breast against the left edge, its centre and axes
varying per image) on exact black.  No real mammogram has been measured; what (c) reports describes these masks and nothing else.

  (a) the two new launches for the whole batch, next to `mmg_patchify_aug` on the same input (it reads the same bytes and writes patch^2 times
      as many values: the yardstick of a kernel that reads every pixel once) and next to `mmg_patch_keep_indices`, for the three pixel kinds,
      without tables and under flip x + flip y with odd shifts.  The 64 images (64 / 128 / 256 MiB) are read again and again from the same
      buffer, so the 256 MiB Infinity Cache serves part of every launch here, of the yardstick's too: compare the columns, not the GB/s with HBM.
  (b) forward + backward and peak memory per rate under both priors: HIP events around windows of `reps` steps, the (rate, prior) cells
      alternating, `rounds` windows each, one untimed step after every change; a fresh seed every step.  Equal K is equal work after the draw.
  (c) per rate and prior, the share of the foreground patches that are kept, from tower.last_patch_foreground for the prior and from the
      uniform draw on the same counts otherwise.

    python tools/patch_prior_cost.py [--batch 64] [--size 1024] [--micro-batch 16] [--reps 2] [--rounds 3] [--dtype uint16] [--out profiles/patch_prior.md]
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
from mmgclip.kernels import PIXEL_KINDS                                         # noqa: E402
from mmgclip.networks.encoder import ViTB16Encoder                              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--micro-batch", type=int, default=16)
ap.add_argument("--layers", type=int, default=12)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--dtype", choices=("uint16", "uint8", "float32"), default="uint16", help="pixel kind the tower is fed in (b)")
ap.add_argument("--threshold", type=float, default=0.0)
ap.add_argument("--min-pixels", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("patch_prior_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")
RATES = (0.25, 0.5, 0.75)
PRIORS = ("uniform", "foreground")
HID, PATCH = 768, 16


def half_ellipses(n, size, seed):
    """fp32 [n, 1, size, size] on the device: inside a half-ellipse against the left edge noise in (0.05, 1], outside exact 0.
    Centre row in [0.4, 0.6] size, half-axes in [0.35, 0.6] size (across) and [0.3, 0.45] size (down), drawn per image."""
    g = torch.Generator().manual_seed(seed)
    cy = (0.4 + 0.2 * torch.rand(n, generator=g)) * size
    ax = (0.35 + 0.25 * torch.rand(n, generator=g)) * size
    ay = (0.3 + 0.15 * torch.rand(n, generator=g)) * size
    y = torch.arange(size, dtype=torch.float32, device=dev)[None, :, None]
    x = torch.arange(size, dtype=torch.float32, device=dev)[None, None, :]
    inside = (x / ax.to(dev)[:, None, None]) ** 2 + ((y - cy.to(dev)[:, None, None]) / ay.to(dev)[:, None, None]) ** 2 <= 1.0
    noise = 0.05 + 0.95 * torch.rand(n, size, size, generator=torch.Generator(device=dev).manual_seed(seed + 1), device=dev)
    return torch.where(inside, noise.clamp_(max=1.0), torch.zeros((), device=dev))[:, None].contiguous()


def as_kind(img01, name):
    if name == "float32":
        return img01
    if name == "uint8":
        return (img01 * 255.0).ceil().to(torch.uint8)                           # (ceil: what is tissue stays above 0)
    v = (img01 * 65535.0).ceil().to(torch.int32)
    return torch.where(v >= 32768, v - 65536, v).to(torch.int16).view(torch.uint16)       # (uint16 is storage only in torch)


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def fmt(v, unit="ms", d=1):
    return f"{statistics.median(v):.{d}f} {unit} (min {min(v):.{d}f}, max {max(v):.{d}f}, {len(v)} windows)"


img01 = half_ellipses(args.batch, args.size, seed=1)
P = (args.size // PATCH) ** 2
KP = (PATCH * PATCH + 31) // 32 * 32

# ---- (a) the launches ------------------------------------------------------------------------------------------------------------------------
rows_a = []
counts = torch.empty(args.batch, P, device=dev, dtype=torch.int32)
p0 = torch.empty(args.batch * P, KP, device=dev, dtype=torch.bfloat16)
flip = torch.tensor([[3, 2 * (i % 9) - 7, 2 * (i % 5) + 1, 0] for i in range(args.batch)], dtype=torch.int32).to(dev)   # both flips, odd shifts
for name in ("uint16", "uint8", "float32"):
    pix = as_kind(img01, name)
    kind, nbytes = PIXEL_KINDS[pix.dtype], pix.numel() * pix.element_size()
    for label, geom in (("no tables", None), ("flip x + flip y, odd shifts", flip)):
        fg = lambda: call("mmg_patch_foreground", ptr(pix), kind, args.batch, 1, args.size, args.size, PATCH, ptr(geom), args.threshold,  # noqa: E731
                          ptr(counts), stream())
        pf = lambda: call("mmg_patchify_aug", ptr(pix), kind, ptr(p0), args.batch, 1, args.size, args.size, PATCH, KP, 1, ptr(geom), None,  # noqa: E731
                          stream())
        timed(fg, 3), timed(pf, 3)
        t_fg = [timed(fg, 20) * 1e3 for _ in range(args.rounds)]
        t_pf = [timed(pf, 20) * 1e3 for _ in range(args.rounds)]
        rows_a.append(f"| {name} | {label} | {nbytes / 2 ** 20:.0f} MiB | {fmt(t_fg, 'us')} | {nbytes / statistics.median(t_fg) / 1e3:.0f} | "
                      f"{fmt(t_pf, 'us')} | {statistics.median(t_fg) / statistics.median(t_pf):.2f} |")
    del pix
del p0
pix = as_kind(img01, args.dtype)                       # what (b) feeds the tower, and the counts (c) looks the uniform draw up in
call("mmg_patch_foreground", ptr(pix), PIXEL_KINDS[pix.dtype], args.batch, 1, args.size, args.size, PATCH, None, args.threshold, ptr(counts),
     stream())
torch.cuda.synchronize()
rows_draw = []
for r in RATES:
    K = PD.keep_count(P, r)
    keep = torch.empty(args.batch, K, device=dev, dtype=torch.int32)
    slot = torch.empty(args.batch, P, device=dev, dtype=torch.int32)
    nfg = torch.empty(args.batch, device=dev, dtype=torch.int32)
    seeds = iter(range(1, 10000))
    plain = lambda: call("mmg_patch_keep_indices", next(seeds), None, args.batch, P, K, ptr(keep), ptr(slot), stream())  # noqa: E731
    prior = lambda: call("mmg_patch_keep_indices_prior", next(seeds), None, ptr(counts), args.min_pixels, args.batch, P, K, ptr(keep),  # noqa: E731
                         ptr(slot), ptr(nfg), stream())
    timed(plain, 3), timed(prior, 3)
    rows_draw.append(f"| {r} | {K} | {fmt([timed(plain, 20) for _ in range(args.rounds)], 'ms', 3)} | "
                     f"{fmt([timed(prior, 20) for _ in range(args.rounds)], 'ms', 3)} |")

# ---- (b), (c) the tower ------------------------------------------------------------------------------------------------------------------------
torch.manual_seed(0)
tower = ViTB16Encoder(image_size=args.size, layers=args.layers, micro_batch=args.micro_batch, patch_threshold=args.threshold,
                      patch_min_pixels=args.min_pixels).to(dev).train()
wgt = torch.randn(args.batch, HID, device=dev)
nfg_all = (counts >= args.min_pixels).sum(1)
share_bg = 1.0 - float(nfg_all.float().mean()) / P


def step():
    tower.zero_grad(set_to_none=True)
    (tower(pix) * wgt).sum().backward()


cells = [(r, p) for r in RATES for p in PRIORS]
ms, peak, kept = {c: [] for c in cells}, {c: 0 for c in cells}, {c: [] for c in cells}
for _ in range(args.rounds):
    for c in cells:
        tower.patch_dropout, tower.patch_prior = c
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms[c].append(timed(step, args.reps))
        peak[c] = max(peak[c], torch.cuda.max_memory_allocated())
        K = PD.keep_count(P, c[0])
        if c[1] == "foreground":
            nfg, k_used = tower.last_patch_foreground
            assert k_used == K and torch.equal(nfg, nfg_all.to(torch.int32))
            kept[c].append(float((torch.clamp(nfg, max=K).float() / nfg.clamp(min=1).float()).mean()))
        else:                                           # the uniform draw of one more seed, looked up in the same counts
            keep = torch.empty(args.batch, K, device=dev, dtype=torch.int32)
            slot = torch.empty(args.batch, P, device=dev, dtype=torch.int32)
            call("mmg_patch_keep_indices", tower._patch_drop_seeds.draw(), None, args.batch, P, K, ptr(keep), ptr(slot), stream())
            hit = (torch.gather(counts, 1, keep.long()) >= args.min_pixels).sum(1)
            kept[c].append(float((hit.float() / nfg_all.clamp(min=1).float()).mean()))

lines = [
    "# The foreground prior of patch dropout: what it costs, what it keeps",
    "",
    f"Box `{socket.gethostname()}`, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; `tools/patch_prior_cost.py`: ViT-B/16 image tower alone "
    f"({args.layers} layers), {args.batch} images of {args.size} x {args.size} (P = {P} patches) in micro-batches of {args.micro_batch}, bf16, "
    f"pixels fed as {args.dtype}; patch_threshold {args.threshold}, patch_min_pixels {args.min_pixels}.",
    "",
    "**The images are synthetic**: a half-ellipse of noise against the left edge on exact black, from the tool's own generator, "
    f"{100 * share_bg:.1f} % of their patches background.  Nobody has measured the background share of a real mammogram here; table (c) "
    "describes these masks and nothing else.",
    "",
    "## (a) The two new launches, whole batch",
    "",
    "`mmg_patch_foreground` next to `mmg_patchify_aug` on the same input in the same process (the same bytes read, patch^2 = 256 times "
    f"fewer values written), HIP events around 20 launches, median (min, max) of {args.rounds} windows.  The same buffer is read again and "
    "again, so the 256 MiB Infinity Cache serves part of every launch, the yardstick's as well: the ratio is the figure, not the GB/s.",
    "",
    "| pixels | geometry | bytes read | `mmg_patch_foreground` | GB/s | `mmg_patchify_aug` | ratio |",
    "|---|---|---|---|---|---|---|",
    *rows_a,
    "",
    "| rate | K | `mmg_patch_keep_indices` | `mmg_patch_keep_indices_prior` |",
    "|---|---|---|---|",
    *rows_draw,
    "",
    "## (b) Forward + backward, (c) share of the foreground patches kept",
    "",
    f"HIP events, windows of {args.reps} steps, the six cells alternating in one process, median (min, max) of {args.rounds} windows each, one "
    "untimed step after every change; a fresh seed every step.  Equal K is equal work after the draw; the uniform prior on the same box in the "
    "same run is the yardstick.  (c): the mean over the images of (foreground patches kept) / (foreground patches), from "
    "`tower.last_patch_foreground` under the prior (min(nfg, K) / nfg) and from a uniform draw looked up in the same counts otherwise.",
    "",
    "| rate | K | prior | forward + backward | against uniform | peak memory | foreground patches kept |",
    "|---|---|---|---|---|---|---|",
]
for r in RATES:
    for p in PRIORS:
        c = (r, p)
        lines.append(f"| {r} | {PD.keep_count(P, r)} | {p} | {fmt(ms[c])} | {statistics.median(ms[c]) / statistics.median(ms[(r, 'uniform')]):.3f} | "
                     f"{peak[c] / 2 ** 30:.2f} GiB | {100 * statistics.mean(kept[c]):.1f} % |")
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
