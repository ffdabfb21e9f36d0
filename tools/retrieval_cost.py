#!/usr/bin/env python3
"""What the retrieval metrics cost at validation-set size, D = 512 and N = 2048 / 8192 / 16384 on one device:

  * the fused rank kernel (`head._HipRetrievalBackend.rank`), both directions, on the diagonal and with keys shared by groups of four;
  * the dense torch route to the same four vectors on the same device (`X @ Y.T`, masks, comparisons, sums), and its peak memory;
  * the kernel route's peak memory, checked against the claim that can be derived: 4 x 4 N bytes of outputs per direction and no
    [N,N] allocation (`torch.cuda.max_memory_allocated` above the inputs);
  * one `ClassifierExperiment.validate()` with and without `experiments.config.retrieval` on the synthetic `train_prompt_clf` set.

HIP events around single calls (host clock around validate(), which ends in a synchronise), the variants alternating, median (min, max).

    python tools/retrieval_cost.py [--reps 10] [--warmup 2] [--sizes 2048 8192 16384] [--val-batches 16] [--out profiles/retrieval.md]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import torch                                                                    # noqa: E402
from mmgclip import head                                                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 8192, 16384])
ap.add_argument("--val-batches", type=int, default=16)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("retrieval_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")
ARCH = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
PART = (f"MI355X ({ARCH}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)" if ARCH == "gfx950"
        else f"{torch.cuda.get_device_name(0)} ({ARCH})")
D = 512


def fused(img, txt, labels):
    return [head._HipRetrievalBackend.rank(x, y, labels, labels, 0) for x, y in ((img, txt), (txt, img))]


def dense(img, txt, labels):
    out = []
    N = img.shape[0]
    idx = torch.arange(N, device=img.device)
    for x, y in ((img, txt), (txt, img)):
        s = x @ y.t()
        pos = (idx[None, :] == idx[:, None]) if labels is None else (labels[None, :] == labels[:, None])
        best = torch.where(pos, s, torch.full_like(s, float("-inf"))).max(dim=1).values
        neg = ~pos
        out.append((best, pos.sum(1), (neg & (s > best[:, None])).sum(1), (neg & (s == best[:, None])).sum(1)))
    return out


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


kernel_rows, memory_rows = [], []
for N in args.sizes:
    g = torch.Generator().manual_seed(N)
    img = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).to(dev)
    txt = torch.nn.functional.normalize(img.cpu() + 0.8 * torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1), dim=1).to(dev)
    for mode, labels in (("diagonal", None), ("keys, groups of 4", (torch.arange(N, device=dev) // 4).contiguous())):
        variants = {"fused": lambda: fused(img, txt, labels), "dense": lambda: dense(img, txt, labels)}
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
        claim = 2 * 4 * 4 * N                                     # two directions x four [N] vectors of 4 bytes
        assert mem["fused"] < 2 * claim + 8 * 512 and mem["fused"] < N * N * 4 // 64, (mem, claim)
        f, d = fused(img, txt, labels), dense(img, txt, labels)
        same = min(float(((a[2] + a[3]) == (b[2] + b[3])).double().mean()) for a, b in zip(f, d))
        assert all(torch.equal(a[1].long(), b[1]) for a, b in zip(f, d))
        sweeps = 1 if labels is None else 2                       # on the diagonal sweep 1 visits one or two tiles per workgroup
        flop = 2 * sweeps * 2.0 * N * N * D                       # two directions
        kernel_rows.append(f"| {N} | {mode} | {fmt(t['fused'])} | {flop / statistics.median(t['fused']) / 1e9:.1f} | {fmt(t['dense'])} | "
                           f"{statistics.median(t['dense']) / statistics.median(t['fused']):.2f}x | {same:.4f} |")
        memory_rows.append(f"| {N} | {mode} | {mem['fused']} | {claim} | {mem['dense']} ({mem['dense'] / 2 ** 20:.0f} MiB) | {N * N * 4} |")
    del img, txt
    torch.cuda.empty_cache()


# ---- one validate() with and without the key ------------------------------------------------------------------------------------
def experiment(extra):
    from mmgclip.config import compose
    from mmgclip.dataset.synthetic import SyntheticLoader
    from mmgclip.experiments.experiments_controller import create_experiment
    tmp = tempfile.mkdtemp(prefix="retrieval_cost_")
    cfg = compose(os.path.join(ROOT, "mmg-clip_amd", "configs"), "train_prompt_clf", ["networks.text_encoder.random_init=true"] + extra)
    cfg.checkpoints.checkpoints_export_dir = os.path.join(tmp, "ckpt")
    cfg.base.tensorboard_export_dir = os.path.join(tmp, "tb")
    torch.manual_seed(0)
    bs, S = cfg.dataloader.valid.batch_size, cfg.tokenizer.config.sequence_length
    return create_experiment("classification")(config=cfg, train_dataloader=[], valid_dataloader=SyntheticLoader(args.val_batches, bs, seed=9, S=S),
                                               test_dataloader=None, tokenizer=None), bs


def validate_s(exp):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    val = exp.validate()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, val


exps = {"without the key": experiment([])[0]}
exps["with the key (`+experiments/config/retrieval=recall`)"], bs = experiment(["+experiments/config/retrieval=recall"])
for e in exps.values():
    validate_s(e)
tv = {name: [] for name in exps}
order = list(exps)
for rep in range(max(3, args.reps // 3)):
    for name in (order if rep % 2 == 0 else order[::-1]):
        tv[name].append(validate_s(exps[name])[0] * 1e3)
n_val = args.val_batches * bs
retr = exps[order[1]].retrieval
val_rows = [f"| {name} | {fmt(tv[name])} |" for name in order]

lines = [
    "# Retrieval metrics at validation: the fused rank kernel against the dense route",
    "",
    f"{PART}, torch {torch.__version__}; `tools/retrieval_cost.py`: D = {D}, N queries against N gallery rows, both directions (i2t and t2i) "
    f"per figure, one process.  HIP events around single calls, {args.warmup} warm-up and {args.reps} timed calls of each variant, the order "
    "alternating; ms, median (min, max).  `fused` is `mmg_retrieval_rows_rank` twice (one launch per direction, two sweeps each); TFLOP/s "
    "counts `2 N N D` FLOP per full sweep and direction - two full sweeps with keys, one on the diagonal, where sweep 1 visits only the one "
    "or two tiles that hold a workgroup's positives - and is a whole-call rate, not a share of peak.  `dense` is `X @ Y.T`, the positive mask, "
    "`where/max`, two comparisons and three row sums in torch on the same device.  `same rank` is the smallest share, over the two "
    "directions, of queries to which the two routes give the same rank; they form the dot products in different orders, so on random unit "
    "rows a score within rounding of the threshold may fall on either side (the tests compare the kernel with float64 intervals instead).",
    "",
    "| N | positives | fused | TFLOP/s | dense | dense / fused | same rank |",
    "|---|---|---|---|---|---|---|",
] + kernel_rows + [
    "",
    "## Memory",
    "",
    "Peak of `torch.cuda.max_memory_allocated` above the inputs, results alive, bytes.  The claim that can be derived - `4 x 4 N` bytes of "
    "outputs per direction and no `[N,N]` allocation - is asserted by the tool (`fused` below twice the claim and below 1/64 of one fp32 "
    "`[N,N]`).",
    "",
    "| N | positives | fused peak | claim (2 x 4 x 4 N) | dense peak | one fp32 [N,N] |",
    "|---|---|---|---|---|---|",
] + memory_rows + [
    "",
    "## One validate()",
    "",
    f"`train_prompt_clf` as shipped (pre-extracted image features, BERT-base with random weights, `1xLinear512`), the synthetic loader: "
    f"{args.val_batches} batches of {bs} = {n_val} pairs; host clock around `validate()` ending in a synchronise, one warm-up, the two "
    "experiments alternating; ms, median (min, max).  The synthetic reports are all different, so `positives: text` finds no duplicates here; "
    "the work is the same.",
    "",
    "| validate() | ms |",
    "|---|---|",
] + val_rows + [
    "",
    f"`self.retrieval` of the last run (random weights): " + ", ".join(f"{k} {v:.4g}" for k, v in retr.items()),
]
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
