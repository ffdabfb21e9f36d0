#!/usr/bin/env python3
"""What clipping the gradients by their global norm (and guarding the step against NaN / Inf) costs on buffers of the C2 step's
sizes: a ConvNeXt-T arena, a BERT-base arena and the head tensors (two 768 -> 512 projections, logit_scale).  HIP events around
single calls, 2 warm-up and 10 timed repetitions of each variant, the variants alternating:

  (a) FusedAdamW.step() as it has always been (max_grad_norm=None: one mmg_adamw_step launch per arena and per loose tensor)
  (b) FusedAdamW.step() with max_grad_norm=1.0 (mmg_grad_sumsq per piece, mmg_grad_clip_finalize, mmg_adamw_step_guarded)
  (c) the reduction launches of (b) alone

The bar: (b) <= (a) + (c) + 10 % (launch latency of the loose tensors, run-to-run spread).

    python tools/grad_clip_cost.py [--reps 10] [--warmup 2] [--out profiles/r06_grad_clip.md]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import torch                                                                    # noqa: E402
from mmgclip import kernels as K                                                # noqa: E402
from mmgclip.optim import FusedAdamW                                            # noqa: E402
from mmgclip.params import ParamArena                                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("grad_clip_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")
# torch may report the marketing name of the part generically ("AMD Radeon Graphics"): name it by its architecture
ARCH = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
PART = (f"MI355X ({ARCH}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)" if ARCH == "gfx950"
        else f"{torch.cuda.get_device_name(0)} ({ARCH})")

# parameter counts of the C2 step (bench.py's default workload): torchvision ConvNeXt-T without its classifier and with a 1-channel
# stem, Bio_ClinicalBERT (BERT-base, 28996-token vocabulary); an arena is one flat buffer whatever the tensors inside it are
TOWERS = {"convnext_tiny": 27_815_424, "bert_base": 108_310_272}
HEADS = [(512, 768), (512, 768), ()]


def build(**kw):
    arenas, params = [], []
    for name, total in TOWERS.items():
        named = [(f"{name}.{i}", torch.nn.Parameter(torch.randn(total // 8) * 0.02)) for i in range(8)]
        arenas.append(ParamArena(named, dev))
        params += arenas[-1].params
    loose = [torch.nn.Parameter((torch.randn(s) * 0.02).to(dev)) for s in HEADS]
    g = torch.Generator(device=dev).manual_seed(1)
    for a in arenas:
        a.grad.copy_(torch.randn(a.size, device=dev, generator=g) * 1e-3)
        for n, p in zip(a.names, a.params):
            p.grad = a.g(n)
    for p in loose:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    return FusedAdamW(params + loose, lr=5e-5, weight_decay=1e-4, **kw), arenas, loose


plain, _, _ = build()
guarded, g_arenas, g_loose = build(max_grad_norm=1.0)
pieces = [a.grad for a in g_arenas] + [p.grad for p in g_loose]
counts = [K.grad_sumsq_partials(t.numel()) for t in pieces]
partials = torch.empty(sum(counts), device=dev, dtype=torch.float64)
out = torch.zeros(4, device=dev)
skipped = torch.zeros(1, device=dev, dtype=torch.int32)


def reduce_only():
    off = 0
    for t, c in zip(pieces, counts):
        K.grad_sumsq(t, partials, off, c)
        off += c
    K.grad_clip_finalize(partials, off, 1.0, out, skipped)


VARIANTS = {"plain": plain.step, "guarded": guarded.step, "reduce": reduce_only}
for fn in VARIANTS.values():
    for _ in range(args.warmup):
        fn()
torch.cuda.synchronize()
times = {name: [] for name in VARIANTS}
for _ in range(args.reps):
    for name, fn in VARIANTS.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times[name].append(s.elapsed_time(e))
norm, coef, finite, _ = guarded.grad_norm.tolist()
assert finite == 1.0 and guarded.skipped_steps() == 0 and coef < 1.0, (norm, coef, finite)


def fmt(ms):
    return f"{statistics.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} calls)"


n_elem = sum(t.numel() for t in pieces)
med = {k: statistics.median(v) for k, v in times.items()}
bar = (med["plain"] + med["reduce"]) * 1.10
lines = [
    "# Gradient clipping by global norm: what the guarded optimizer step costs",
    "",
    f"{PART}, torch {torch.__version__}; `tools/grad_clip_cost.py`: a ConvNeXt-T arena ({TOWERS['convnext_tiny']:,} fp32), a BERT-base arena "
    f"({TOWERS['bert_base']:,}) and the head tensors (two 512 x 768 projections, logit_scale): {n_elem:,} gradient elements = {4 * n_elem / 1e9:.3f} GB.  "
    f"HIP events around single calls, {args.warmup} warm-up and {args.reps} timed calls of each variant, the variants alternating; median (min, max).",
    "",
    "| | what | time |",
    "|---|---|---|",
    f"| (a) | `FusedAdamW.step()`, `max_grad_norm=None`: {len(pieces)} `mmg_adamw_step` launches | {fmt(times['plain'])} |",
    f"| (b) | `FusedAdamW.step()`, `max_grad_norm=1.0`: {len(pieces)} `mmg_grad_sumsq` + `mmg_grad_clip_finalize` + {len(pieces)} `mmg_adamw_step_guarded` | {fmt(times['guarded'])} |",
    f"| (c) | the reduction launches of (b) alone ({sum(counts)} fp64 partials) | {fmt(times['reduce'])} |",
    "",
    f"(c) reads {4 * n_elem / 1e9:.3f} GB in {med['reduce']:.3f} ms = {4 * n_elem / 1e9 / med['reduce']:.2f} TB/s.  "
    f"(b) - (a) = {med['guarded'] - med['plain']:+.3f} ms.  The bar, (a) + (c) + 10 % = {bar:.3f} ms: (b) is "
    f"{'within' if med['guarded'] <= bar else 'ABOVE'} it.  Last guarded step: norm {norm:.4f}, coefficient {coef:.4f}.",
]
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
