#!/usr/bin/env python3
"""What the fine-tuning recipe's param groups (no-decay set + layer-wise lr decay) cost in the optimizer step, on arenas of the C2 step's
sizes and tensor counts: a ConvNeXt-T arena (180 tensors, 19 layer ids), a BERT-base arena (199 tensors, 14 layer ids) and the head
tensors.  Three optimizers over buffers of their own, in the same process, HIP events around single `step()` calls, the variants
alternating inside every round:

  (a) FusedAdamW.step() over ONE group, as it has always been: one mmg_adamw_step launch per arena and per loose tensor
  (b) the grouped recipe on the per-tensor path - what FusedAdamW did with these groups before mmg_adamw_step_groups existed: one
      mmg_adamw_step launch per tensor
  (c) the grouped recipe, one mmg_adamw_step_groups launch per arena

(a) is reported per round (5 rounds by default): the spread of its round medians is the yardstick.  The bar: (c) within that spread of
(a) or faster, and below (b).

    python tools/adamw_groups_cost.py [--rounds 5] [--reps 10] [--warmup 2] [--out profiles/r08_adamw_groups.md]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import torch                                                                    # noqa: E402
from mmgclip.optim import FusedAdamW                                            # noqa: E402
from mmgclip.params import ParamArena                                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("adamw_groups_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")
ARCH = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
PART = (f"MI355X ({ARCH}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)" if ARCH == "gfx950"
        else f"{torch.cuda.get_device_name(0)} ({ARCH})")

# element counts as in tools/grad_clip_cost.py; tensor and layer counts of the two towers (ConvNeXt-T: 180 parameters, stem + 18 blocks;
# BERT-base: 199 parameters, embeddings + 12 layers + pooler).  What a tensor holds does not matter to the step, how many there are does.
TOWERS = {"convnext_tiny": (27_815_424, 180, 19), "bert_base": (108_310_272, 199, 14)}
HEADS = [(512, 768), (512, 768), ()]
LR, WD, DECAY = 5e-5, 1e-4, 0.75


def build(grouped):
    arenas, groups, loose_groups = [], {}, []
    for name, (total, tensors, layers) in TOWERS.items():
        each = total // tensors // 64 * 64
        sizes = [each] * (tensors - 1) + [total - each * (tensors - 1)]
        named = [(f"{name}.{i}", torch.nn.Parameter(torch.randn(s) * 0.02)) for i, s in enumerate(sizes)]
        arena = ParamArena(named, dev)
        arenas.append(arena)
        for i, p in enumerate(arena.params):                      # layer by position, every second tensor a "bias" without weight decay
            layer, plain = i * layers // tensors, i % 2 == 1
            key = (name, layer, plain) if grouped else "all"
            g = groups.setdefault(key, dict(params=[], lr=LR * DECAY ** (layers - 1 - layer) if grouped else LR,
                                            weight_decay=0.0 if grouped and plain else WD))
            g["params"].append(p)
    loose = [torch.nn.Parameter((torch.randn(s) * 0.02).to(dev)) for s in HEADS]
    for p in loose:
        key = ("head", None, p.ndim <= 1) if grouped else "all"
        groups.setdefault(key, dict(params=[], lr=LR, weight_decay=0.0 if grouped and p.ndim <= 1 else WD))["params"].append(p)
    gen = torch.Generator(device=dev).manual_seed(1)
    for a in arenas:
        for n, p in zip(a.names, a.params):
            a.g(n).copy_(torch.randn(p.shape, device=dev, generator=gen) * 1e-3)      # (the padding gaps stay zero)
            p.grad = a.g(n)
    for p in loose:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    return FusedAdamW(list(groups.values()), lr=LR, weight_decay=WD), arenas, loose


single, s_arenas, s_loose = build(False)
per_tensor, _, _ = build(True)
per_tensor._grouped_launch = lambda arena, group_of: None        # the parent commit's answer to a split arena: every tensor a launch
grouped, g_arenas, _ = build(True)
n_groups = len(grouped.param_groups)
n_tensors = sum(len(a.params) for a in s_arenas) + len(s_loose)

VARIANTS = {"single": single.step, "per_tensor": per_tensor.step, "grouped": grouped.step}
for fn in VARIANTS.values():
    for _ in range(args.warmup):
        fn()
torch.cuda.synchronize()
assert all("chunk_map" in grouped._flat[id(a)] for a in g_arenas) and not any("chunk_map" in fs for fs in per_tensor._flat.values())
rounds = {name: [] for name in VARIANTS}
for _ in range(args.rounds):
    times = {name: [] for name in VARIANTS}
    for _ in range(args.reps):
        for name, fn in VARIANTS.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e))
    for name in VARIANTS:
        rounds[name].append(times[name])


def med_of_rounds(name):
    return [statistics.median(r) for r in rounds[name]]


def fmt(name):
    flat = [t for r in rounds[name] for t in r]
    return f"{statistics.median(flat):.3f} ms (min {min(flat):.3f}, max {max(flat):.3f}, {len(flat)} calls)"


n_elem = sum(a.size for a in s_arenas) + sum(p.numel() for p in s_loose)
a_meds = med_of_rounds("single")
a_lo, a_hi = min(a_meds), max(a_meds)
med = {k: statistics.median([t for r in rounds[k] for t in r]) for k in VARIANTS}
within = med["grouped"] <= a_hi
below = med["grouped"] < med["per_tensor"]
gb = 28 * n_elem / 1e9                                                           # p, m, v read and written, g read: seven fp32 passes
lines = [
    "# AdamW with param groups: one launch per arena against a launch per tensor",
    "",
    f"{PART}, torch {torch.__version__}; `tools/adamw_groups_cost.py`: a ConvNeXt-T arena ({TOWERS['convnext_tiny'][0]:,} fp32 in "
    f"{TOWERS['convnext_tiny'][1]} tensors), a BERT-base arena ({TOWERS['bert_base'][0]:,} in {TOWERS['bert_base'][1]}) and the head tensors: "
    f"{n_elem:,} elements, {gb:.3f} GB of fp32 traffic per step (seven passes; the chunk map adds {n_elem / 64 / 1e6:.2f} MB).  The recipe: "
    f"layer-wise lr decay {DECAY} and a no-decay set, {n_groups} param groups.  HIP events around single `step()` calls, {args.warmup} warm-up calls, "
    f"then {args.rounds} rounds of {args.reps} timed calls of each variant, the variants alternating; median (min, max) over all calls.",
    "",
    "| | what | time |",
    "|---|---|---|",
    f"| (a) | one group: {len(s_arenas) + len(s_loose)} `mmg_adamw_step` launches | {fmt('single')} |",
    f"| (b) | {n_groups} groups on the per-tensor path (the parent commit): {n_tensors} `mmg_adamw_step` launches | {fmt('per_tensor')} |",
    f"| (c) | {n_groups} groups, {len(s_arenas)} `mmg_adamw_step_groups` + {len(s_loose)} `mmg_adamw_step` launches | {fmt('grouped')} |",
    "",
    f"(a), median of each round: {', '.join(f'{x:.3f}' for x in a_meds)} ms - spread {a_lo:.3f} ... {a_hi:.3f} ms "
    f"({100 * (a_hi - a_lo) / a_lo:.1f} %).  (c) per round: {', '.join(f'{x:.3f}' for x in med_of_rounds('grouped'))} ms; "
    f"(b) per round: {', '.join(f'{x:.3f}' for x in med_of_rounds('per_tensor'))} ms.",
    "",
    f"(a) moves {gb:.3f} GB in {med['single']:.3f} ms = {gb / med['single']:.2f} TB/s; (c) {gb / med['grouped']:.2f} TB/s.  "
    f"(c) - (a) = {med['grouped'] - med['single']:+.3f} ms; (b) / (c) = {med['per_tensor'] / med['grouped']:.2f}.  The bar - (c) within the "
    f"spread of (a) (<= {a_hi:.3f} ms) or faster, and below (b): (c) is {'within' if within else 'ABOVE'} the spread of (a) and "
    f"{'below' if below else 'NOT below'} (b).",
]
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
