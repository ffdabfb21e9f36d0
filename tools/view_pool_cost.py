#!/usr/bin/env python3
"""What training on whole exams costs: ConvNeXt-T + BERT + CLIPLoss on 64 exams x 4 views of 1024 x 832 (train_exam_reports_clf with
dataset=exam-reports-pixels), the views pooled per exam inside the model (mmgclip/networks/view_pool.py), against the same 256 images as a
flat list without pooling.  HIP events around windows of `reps` calls, after warm-up of every shape; variants alternate, `rounds` windows each.

  (a) the two pooling launches alone (mmg_view_pool_fwd + mmg_view_pool_bwd, V = 256, S = 64, C = 768)
  (b) the same forward + backward as a torch composite on the device (index_add_ / scatter_reduce under autograd)
  (c) the whole training step on the batch of exams (64 reports)
  (d) the whole training step on the 256 images as a flat list, one report per image (what the code could do before exams)
  and, like for like, the image tower alone: forward + backward of (tower + pooling) on the exams and of the tower on the flat list.

    python tools/view_pool_cost.py [--studies 64] [--views 4] [--size 1024 832] [--reps 5] [--rounds 3] [--out profiles/r06_view_pool.md]
"""
import argparse
import os
import socket
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import torch                                                                    # noqa: E402
from mmgclip.config import compose                                              # noqa: E402
from mmgclip.dataset.synthetic import synthetic_batch                           # noqa: E402
from mmgclip.experiments.experiments_controller import create_experiment       # noqa: E402
from mmgclip.networks.view_pool import ViewPool, offsets_to_device, study_offsets   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--studies", type=int, default=64)
ap.add_argument("--views", type=int, default=4)
ap.add_argument("--size", type=int, nargs=2, default=(1024, 832))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("view_pool_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")
S, k, (H, W) = args.studies, args.views, args.size
V = S * k


def window(fn, reps):
    """ms per call over one window of `reps` calls."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def alternate(fns, reps, rounds, warm=2):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            out[name].append(window(fn, reps))
    return out


def fmt(ms, unit="ms"):
    scale = 1000.0 if unit == "us" else 1.0
    return f"{statistics.median(ms) * scale:.2f} {unit} (min {min(ms) * scale:.2f}, max {max(ms) * scale:.2f}, {len(ms)} windows)"


# ---- (a), (b): the pooling step alone ----------------------------------------------------------------------------------------------------
C = 768
feat = torch.randn(V, C, device=dev)
dout = torch.randn(S, C, device=dev)
offs = offsets_to_device(study_offsets([k] * S), dev)
seg = torch.arange(S, device=dev).repeat_interleave(k)
seg2 = seg[:, None].expand(V, C).contiguous()


def hip_pool(mode):
    a = feat.detach().requires_grad_(True)

    def run():
        a.grad = None
        ViewPool.apply(a, offs, S, mode).backward(dout)
    return run


def torch_pool(mode):
    a = feat.detach().requires_grad_(True)

    def run():
        a.grad = None
        if mode == 0:
            out = torch.zeros(S, C, device=dev).index_add_(0, seg, a) / float(k)
        else:
            out = torch.full((S, C), float("-inf"), device=dev).scatter_reduce(0, seg2, a, "amax", include_self=True)
        out.backward(dout)
    return run


pool = alternate({"hip mean": hip_pool(0), "torch mean": torch_pool(0), "hip max": hip_pool(1), "torch max": torch_pool(1)}, 200, args.rounds, warm=20)

# ---- (c), (d): whole steps -------------------------------------------------------------------------------------------------------------------
tmp = tempfile.mkdtemp(prefix="view_pool_cost_")
cfg = compose(os.path.join(ROOT, "mmg-clip_amd", "configs"), "train_exam_reports_clf",
              ["networks=clip_convnexttiny_bert_pixels", "dataset=exam-reports-pixels", "tokenizer=bert_clinical_seqlen=77",
               f"networks.image_encoder.micro_batch={V}", f"dataset.config.n_images_per_study={k}",
               f"checkpoints.checkpoints_export_dir={tmp}/ckpt", f"base.tensorboard_export_dir={tmp}/tb"])
torch.manual_seed(0)
exp = create_experiment(cfg.experiments.config.experiment_name)(config=cfg, train_dataloader=None, valid_dataloader=None,
                                                                test_dataloader=None, tokenizer=None)
exp.model.train()
pix = torch.rand(V, 1, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
VARIANTS = {"exams avgpool": ("avgpool", S), "exams maxpool": ("maxpool", S), "flat list": ("avgpool", V)}   # one model for all three
batches = {}
for name, (method, n_text) in VARIANTS.items():
    b = synthetic_batch(n_text, S=77, seed=2)
    del b["image_features"]
    b["text_tokens"] = b["text_tokens"].to(dev)
    b["image"] = list(pix) if name == "flat list" else [[pix[s * k + j] for j in range(k)] for s in range(S)]
    batches[name] = b


def whole_step(name):
    b = batches[name]

    def run():                                      # the body of ClassifierExperiment.train for one batch
        exp.model.config.dataset.config.concatenate_features_method = VARIANTS[name][0]
        exp.optimizer.zero_grad(set_to_none=True)
        loss, _ = exp.criterion(**exp.model(b))
        loss.backward()
        exp.model.join_streams()
        exp.optimizer.step()
    return run


def tower_step(name):
    b = batches[name]
    wgt = torch.randn(VARIANTS[name][1], 768, device=dev)

    def run():
        exp.model.config.dataset.config.concatenate_features_method = VARIANTS[name][0]
        exp.optimizer.zero_grad(set_to_none=True)
        (exp.model.encode_images(b) * wgt).sum().backward()
    return run


steps = alternate({n: whole_step(n) for n in VARIANTS}, args.reps, args.rounds)
towers = alternate({n: tower_step(n) for n in VARIANTS}, args.reps, args.rounds)

lines = [
    "# Exams from pixels: what pooling the views inside the model costs",
    "",
    f"Box `{socket.gethostname()}`, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; `tools/view_pool_cost.py`: ConvNeXt-T + BERT + CLIPLoss, "
    f"{S} exams x {k} views of {H} x {W} ({V} images, one micro-batch), bf16 towers.  HIP events, windows of {args.reps} steps (200 calls for the "
    f"pooling step alone) after warm-up, variants alternating, median (min, max) of {args.rounds} windows each.",
    "",
    "| | what | time |",
    "|---|---|---|",
    f"| (a) | the two pooling launches, mean: `mmg_view_pool_fwd` + `mmg_view_pool_bwd` through autograd, V = {V}, S = {S}, C = 768 | {fmt(pool['hip mean'], 'us')} |",
    f"| (a) | the same, max | {fmt(pool['hip max'], 'us')} |",
    f"| (b) | torch composite on the device, mean (`index_add_`, division, autograd) | {fmt(pool['torch mean'], 'us')} |",
    f"| (b) | torch composite on the device, max (`scatter_reduce` amax, autograd) | {fmt(pool['torch max'], 'us')} |",
    f"| (c) | whole training step on {S} exams, avgpool ({S} reports) | {fmt(steps['exams avgpool'])} |",
    f"| (c) | whole training step on {S} exams, maxpool ({S} reports) | {fmt(steps['exams maxpool'])} |",
    f"| (d) | whole training step on the same {V} images as a flat list, no pooling ({V} reports) | {fmt(steps['flat list'])} |",
    f"| | image tower + pooling alone, forward + backward, avgpool | {fmt(towers['exams avgpool'])} |",
    f"| | image tower + pooling alone, forward + backward, maxpool | {fmt(towers['exams maxpool'])} |",
    f"| | image tower alone on the flat list, forward + backward | {fmt(towers['flat list'])} |",
    "",
    f"(a) and (b) include autograd's own bookkeeping on the host, the same on both sides.  (d) runs the text tower and the loss on {V} reports where "
    f"(c) runs them on {S}; the tower rows compare the image side like for like.  The spread of (d) is its (min, max).",
]
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
