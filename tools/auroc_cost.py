#!/usr/bin/env python3
"""What the zero-shot AUROC with bootstrap intervals costs on one device, n = 2048 / 16384 / 65536 samples at 10 % positives, B = 1000:

  * the device route: `mmg_bootstrap_weights` and `mmg_auroc_pairs` on one chunk of replicates as `ZeroShotAUROC.compute()` sizes it
    (achieved i8 operations per second and the bytes of weights the pair kernel streams), and the whole `compute()` of one binary task;
  * the host loop of `Evaluator.zeroshot_label_prompt` on the same scores (np.random.choice + sklearn's roc_auc_score per replicate),
    timed on `--host-replicates` replicates and scaled to B;
  * `torch.cuda.max_memory_allocated` of `compute()` above its inputs, against `max_weight_bytes`;
  * one `ClassifierExperiment.validate()` with and without `experiments.config.zeroshot_auroc`;
  * `python bench.py` on this tree and, with `--bench-parent DIR`, on a build of the parent commit in DIR, alternating.

    python tools/auroc_cost.py [--reps 10] [--warmup 2] [--sizes 2048 16384 65536] [--out profiles/auroc.md] [--bench-parent DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import numpy as np                                                              # noqa: E402
import torch                                                                    # noqa: E402
from mmgclip import head, zeroshot_auroc                                        # noqa: E402
from mmgclip._hip import call, ptr, stream                                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 16384, 65536])
ap.add_argument("--replicates", type=int, default=1000)
ap.add_argument("--host-replicates", type=int, default=20)
ap.add_argument("--val-batches", type=int, default=16)
ap.add_argument("--bench-parent", default=None)
ap.add_argument("--bench-steps", type=int, default=20)
ap.add_argument("--bench-rounds", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("auroc_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")
ARCH = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
PART = (f"MI355X ({ARCH}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)" if ARCH == "gfx950"
        else f"{torch.cuda.get_device_name(0)} ({ARCH})")
B, SEED = args.replicates, 0
CAP = 64 << 20


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    del out
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(fn, clock):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    return [clock(fn) for _ in range(args.reps)]


def fmt(ms):
    return f"{statistics.median(ms):.3f} ({min(ms):.3f}, {max(ms):.3f})"


def host_loop(y_true, pos, replicates):
    """evaluator.py's loop, verbatim."""
    from sklearn import metrics
    scores = []
    for _ in range(replicates):
        indices = np.random.choice(len(pos), len(pos), replace=True)
        if len(np.unique(y_true[indices])) == 2:
            scores.append(metrics.roc_auc_score(y_true[indices] == 1, pos[indices]))
    return scores


kernel_rows, route_rows, memory_rows = [], [], []
for n in args.sizes:
    g = np.random.default_rng(n)
    y = np.zeros(n, dtype=np.int64)
    y[g.permutation(n)[:n // 10]] = 1
    s = (g.standard_normal(n) + y).astype(np.float32)
    P, Nn = int(y.sum()), int(n - y.sum())
    ld = (n + 15) // 16 * 16
    chunk = min(B, zeroshot_auroc.replicates_per_chunk(n, CAP))      # as ZeroShotAUROC.compute() sizes it
    sd, yd = torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)
    pos, neg = torch.nonzero(yd == 1).flatten(), torch.nonzero(yd != 1).flatten()
    s_pos, s_neg = sd[pos].contiguous(), sd[neg].contiguous()
    w = head._HipAurocBackend.bootstrap_weights(SEED, n, 0, chunk, dev)
    w_pos, w_neg = zeroshot_auroc._pad16(w.index_select(1, pos)), zeroshot_auroc._pad16(w.index_select(1, neg))
    partial = torch.empty(((P + 31) // 32, chunk), device=dev, dtype=torch.int64)
    t_w = timed(lambda: head._HipAurocBackend.bootstrap_weights(SEED, n, 0, chunk, dev), event_ms)
    t_p = timed(lambda: call("mmg_auroc_pairs", ptr(s_pos), ptr(s_neg), ptr(w_pos), w_pos.shape[1], ptr(w_neg), w_neg.shape[1], P, Nn,
                             chunk, ptr(partial), stream()), event_ms)
    macs = float(P) * Nn * chunk
    streamed = ((P + 31) // 32) * chunk * w_neg.shape[1] + chunk * w_pos.shape[1]
    kernel_rows.append(f"| {n} | {P} x {Nn} | {chunk} | {fmt(t_w)} | {fmt(t_p)} | {2 * macs / statistics.median(t_p) / 1e9:.1f} | "
                       f"{streamed / 2 ** 20:.0f} | {streamed / statistics.median(t_p) / 1e6:.0f} |")
    del w, w_pos, w_neg, partial

    def compute():
        z = zeroshot_auroc.ZeroShotAUROC(n_bootstrap=B, seed=SEED, max_weight_bytes=CAP)
        z.update("task", sd[:, None], yd, [1])
        return z.compute()
    t_c = timed(compute, wall_ms)
    host_loop(y, s, 1)                                              # (sklearn's import and first call are not part of the loop's cost)
    t0 = time.perf_counter()
    host = host_loop(y, s, args.host_replicates)
    t_h = (time.perf_counter() - t0) * 1e3 / args.host_replicates * B
    out = compute()["task"]
    route_rows.append(f"| {n} | {fmt(t_c)} | {t_h:.0f} | {t_h / statistics.median(t_c):.1f}x | {out['auc']:.4f} [{out['ci_lower']:.4f}, "
                      f"{out['ci_upper']:.4f}] | {np.mean(host):.4f} |")
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    compute()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    memory_rows.append(f"| {n} | {chunk} | {peak} ({peak / 2 ** 20:.1f} MiB) | {CAP} ({CAP >> 20} MiB) | {'yes' if peak <= CAP else 'NO'} |")
    del sd, yd, s_pos, s_neg
    torch.cuda.empty_cache()


# ---- one validate() with and without the key ------------------------------------------------------------------------------------
def experiment(extra):
    from mmgclip.config import compose
    from mmgclip.dataset.synthetic import SyntheticLoader
    from mmgclip.experiments.experiments_controller import create_experiment
    tmp = tempfile.mkdtemp(prefix="auroc_cost_")
    cfg = compose(os.path.join(ROOT, "mmg-clip_amd", "configs"), "train_prompt_clf", ["networks.text_encoder.random_init=true"] + extra)
    cfg.checkpoints.checkpoints_export_dir = os.path.join(tmp, "ckpt")
    cfg.base.tensorboard_export_dir = os.path.join(tmp, "tb")
    torch.manual_seed(0)
    bs, S = cfg.dataloader.valid.batch_size, cfg.tokenizer.config.sequence_length
    return create_experiment("classification")(config=cfg, train_dataloader=[], valid_dataloader=SyntheticLoader(args.val_batches, bs, seed=9, S=S),
                                               test_dataloader=None, tokenizer=None), bs


exps = {"without the key": experiment([])[0]}
exps["with the key (`+experiments/config/zeroshot_auroc=bootstrap`)"], bs = experiment(["+experiments/config/zeroshot_auroc=bootstrap"])
for e in exps.values():
    e.validate()
tv = {name: [] for name in exps}
order = list(exps)
for rep in range(max(3, args.reps // 3)):
    for name in (order if rep % 2 == 0 else order[::-1]):
        tv[name].append(wall_ms(exps[name].validate))
zs = exps[order[1]].zeroshot
val_rows = [f"| {name} | {fmt(tv[name])} |" for name in order]
del exps
torch.cuda.empty_cache()


# ---- bench.py on this tree and on the parent's -----------------------------------------------------------------------------------
def bench(tree):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "5"], cwd=tree,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f"bench.py failed in {tree} (exit {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


trees = {"this commit": ROOT}
if args.bench_parent:
    trees["parent commit"] = os.path.abspath(args.bench_parent)
bench_runs = {name: [] for name in trees}
for rnd in range(args.bench_rounds):
    for name in (list(trees) if rnd % 2 == 0 else list(trees)[::-1]):
        bench_runs[name].append(bench(trees[name]))
keys = [k for k, v in bench_runs["this commit"][0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)]
bench_rows = [f"| {name} | " + " | ".join(json.dumps({k: r[k] for k in keys}) for r in runs) + " |" for name, runs in bench_runs.items()]

lines = [
    "# Zero-shot AUROC with bootstrap intervals: the i8 pair-count kernel against the host loop",
    "",
    f"{PART}, torch {torch.__version__}; `tools/auroc_cost.py`: n samples, 10 % positives, B = {B} replicates, one binary task, one process.  "
    f"{args.warmup} warm-up and {args.reps} timed calls; ms, median (min, max).",
    "",
    "## The kernels, one chunk of replicates",
    "",
    "`chunk` is the number of replicates `ZeroShotAUROC.compute()` takes at a time under `max_weight_bytes` = 64 MiB.  HIP events around one "
    "call.  `weights` is `mmg_bootstrap_weights` for the chunk; `pairs` is one `mmg_auroc_pairs` launch on the chunk's gathered columns.  "
    "T i8 op/s counts `2 P Nn chunk` operations over the pairs call (a whole-call rate, not a share of peak).  `streamed` is what the pair "
    "kernel reads of the weights: the negative columns once per 32 positives, the positive columns once.",
    "",
    "| n | P x Nn | chunk | weights | pairs | T i8 op/s | streamed MiB | streamed GB/s |",
    "|---|---|---|---|---|---|---|---|",
] + kernel_rows + [
    "",
    "## The route: device compute() against the host loop",
    "",
    f"`device` is the host clock around `ZeroShotAUROC(n_bootstrap={B}).compute()` ending in a synchronise: weights, column gathers, pair "
    f"kernel, the read-back and {B} Python divisions.  `host` is the loop of `Evaluator.zeroshot_label_prompt` (np.random.choice and "
    f"sklearn's roc_auc_score per replicate) on the same scores, timed once on {args.host_replicates} replicates after one untimed one and scaled to {B}.  The two "
    "draw different resamples (the host's are unseeded), so the intervals agree only statistically.",
    "",
    "| n | device ms | host ms (scaled) | host / device | device auc [ci] | host mean |",
    "|---|---|---|---|---|---|",
] + route_rows + [
    "",
    "## Memory",
    "",
    "Peak of `torch.cuda.max_memory_allocated` during `compute()` above what is live before it (the scores and targets), bytes.",
    "",
    "| n | chunk | peak | max_weight_bytes | within |",
    "|---|---|---|---|---|",
] + memory_rows + [
    "",
    "## One validate()",
    "",
    f"`train_prompt_clf` as shipped, BERT-base with random weights, the synthetic loader: {args.val_batches} batches of {bs}; host clock "
    "around `validate()` ending in a synchronise, one warm-up, the two experiments alternating; ms, median (min, max).",
    "",
    "| validate() | ms |",
    "|---|---|",
] + val_rows + [
    "",
    "`self.zeroshot` of the last run (random weights): " + ", ".join(
        f"{k} {v['auc']:.4f} [{v.get('ci_lower', float('nan')):.4f}, {v.get('ci_upper', float('nan')):.4f}]" for k, v in (zs or {}).items()),
    "",
    "## bench.py",
    "",
    f"`python bench.py --gpus 1 --steps {args.bench_steps} --warmup 5`, {args.bench_rounds} runs per tree, the trees alternating; the numeric "
    "fields of each run's JSON line.  No shipped config sets the key, so the step does not run any of the new code.",
    "",
    "| tree | " + " | ".join(f"run {i + 1}" for i in range(args.bench_rounds)) + " |",
    "|---|" + "---|" * args.bench_rounds,
] + bench_rows
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
