#!/usr/bin/env python3
"""What raw pixels and the in-kernel augmentation cost, on the device, in one process, the variants alternating inside every round.

  (a) kernel: the stem's patchify (Cin = 1, P = 4, Kp = 32, scale16) at [64, 1, 1024, 1024] and [64, 1, 1906, 818]:
        fp32      `mmg_patchify` on fp32 pixels                                   (8 bytes per pixel: 4 in, 4 out)
        u16       `mmg_patchify_aug` on uint16 pixels, NULL tables               (6 bytes per pixel: 2 in, 4 out)
        u16_aug   the same with flips, an odd shift and tone on every image
      HIP events around single launches; microseconds and GB/s of the bytes the kernel must move.  fp32 is reported per round: the spread
      of its round medians is the yardstick for "no slower".
  (b) step: C2-shaped training steps (ConvNeXt-T on 1024 x 1024 pixels + BERT, S = 77, forward + backward + FusedAdamW), the batch's pixels
      on the host (pinned when the allocator allows it) and copied to the device inside every timed step:
        fp32 | u16 | u16 + the example augmentation (configs/networks/image_encoder/augment/mammo.yaml)

    python tools/pixel_input_cost.py [--part kernel|step|all] [--batch 256] [--micro-batch 64] [--rounds 5] [--reps 20] [--out profiles/r09_pixel_input.md]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import torch                                                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=["kernel", "step", "all"])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--micro-batch", type=int, default=64)
ap.add_argument("--step-rounds", type=int, default=4)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("pixel_input_cost.py measures on the GPU: no device found, nothing measured")
dev = torch.device("cuda:0")
ARCH = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
PART = (f"MI355X ({ARCH}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)" if ARCH == "gfx950"
        else f"{torch.cuda.get_device_name(0)} ({ARCH})")
from mmgclip import augment as A                                                # noqa: E402
from mmgclip import kernels as K                                                # noqa: E402

lines = ["# Raw 8/16-bit pixels and augmentation in the stem's patchify: what they cost", "",
         f"{PART}, torch {torch.__version__}; `tools/pixel_input_cost.py`, one process, the variants alternating inside every round.", ""]


def med(xs):
    return statistics.median(xs)


def kernel_part():
    lines.extend(["## (a) the kernel", "",
                  f"Cin = 1, P = 4, Kp = 32, scale16 on.  HIP events around single launches, {args.warmup} warm-up launches of every variant, then "
                  f"{args.rounds} rounds of {args.reps} timed launches each, alternating; median (min, max) over all launches.  GB/s = the bytes the "
                  "kernel must move (pixels in at their width + 64 bytes per 4 x 4 patch out) over the median.", ""])
    for n, H, W in ((64, 1024, 1024), (64, 1906, 818)):
        host = torch.rand(n, 1, H, W, generator=torch.Generator().manual_seed(1))        # (uint16 is storage only in torch: converted on the host)
        u16_host = (host * 65535).round().to(torch.int32).to(torch.uint16)
        f32, u16 = host.to(dev), u16_host.to(dev)
        as_float = (u16_host.to(torch.int32).to(torch.float32) / 65535.0).to(dev)
        spec = A.AugmentSpec(hflip=1.0, vflip=1.0, max_shift=0, gain=(0.9, 1.1), offset=(-0.05, 0.05))
        geom, tone = A.draw(spec, 5, range(n))
        for i, r in enumerate(geom):                       # flips on every image, odd shifts (misaligned reads on every row)
            r[1], r[2] = 2 * (i % 9) - 7, 2 * (i % 11) - 9
        geom_d = torch.tensor(geom, dtype=torch.int32, device=dev)
        tone_d = torch.tensor(tone, dtype=torch.float32, device=dev)
        variants = {"fp32": lambda: K.patchify(f32, 4, 32, True), "u16": lambda: K.patchify(u16, 4, 32, True),
                    "u16_aug": lambda: K.patchify(u16, 4, 32, True, geom_d, tone_d)}
        same = torch.equal(K.patchify(u16, 4, 32, True), K.patchify(as_float, 4, 32, True))
        del as_float, host, u16_host
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in variants}
        for _ in range(args.rounds):
            t = {k: [] for k in variants}
            for _ in range(args.reps):
                for k, fn in variants.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    fn()
                    e.record()
                    torch.cuda.synchronize()
                    t[k].append(s.elapsed_time(e) * 1e3)
            for k in variants:
                rounds[k].append(t[k])
        px = n * H * W
        out_bytes = n * (H // 4) * (W // 4) * 64
        nbytes = {"fp32": 4 * px + out_bytes, "u16": 2 * px + out_bytes, "u16_aug": 2 * px + out_bytes}
        what = {"fp32": "`mmg_patchify`, fp32 pixels", "u16": "`mmg_patchify_aug`, uint16 pixels, no tables",
                "u16_aug": "`mmg_patchify_aug`, uint16, flip x + flip y, odd shifts, tone on every image"}
        lines.extend([f"### [{n}, 1, {H}, {W}]", "", "| variant | microseconds | GB/s | bytes |", "|---|---|---|---|"])
        m = {}
        for k in variants:
            flat = [x for r in rounds[k] for x in r]
            m[k] = med(flat)
            lines.append(f"| {what[k]} | {m[k]:.1f} (min {min(flat):.1f}, max {max(flat):.1f}, {len(flat)} launches) | "
                         f"{nbytes[k] / m[k] / 1e3:.0f} | {nbytes[k] / 2 ** 20:.0f} MiB |")
        fm = [med(r) for r in rounds["fp32"]]
        lines.extend(["", f"fp32, median of each round: {', '.join(f'{x:.1f}' for x in fm)} us - spread {min(fm):.1f} ... {max(fm):.1f} us "
                      f"({100 * (max(fm) - min(fm)) / min(fm):.1f} %).  u16 per round: {', '.join(f'{med(r):.1f}' for r in rounds['u16'])} us; "
                      f"u16_aug per round: {', '.join(f'{med(r):.1f}' for r in rounds['u16_aug'])} us.",
                      f"The identity uint16 launch is {'no slower than' if m['u16'] <= max(fm) else 'SLOWER than'} the fp32 launch beyond the fp32 "
                      f"launch's own spread (u16 / fp32 = {m['u16'] / m['fp32']:.3f}; u16_aug / u16 = {m['u16_aug'] / m['u16']:.3f}).  "
                      f"uint16 output == fp32-kernel output on v / 65535, bit for bit, at this size: {same}.", ""])
        del f32, u16
        torch.cuda.empty_cache()


def step_part():
    from mmgclip.config import compose
    from mmgclip.dataset.synthetic import as_pixel_dtype, synthetic_batch
    from mmgclip.loss.loss_controller import create_loss
    from mmgclip.networks.mmgclip_model import MMGCLIP
    from mmgclip.optim import FusedAdamW
    from mmgclip.utils.global_utils import seeding
    cfg_dir = os.path.join(ROOT, "mmg-clip_amd", "configs")
    cfg = compose(cfg_dir, "train_binary_class_clf",
                  ["networks=clip_convnexttiny_bert_pixels", "tokenizer=bert_clinical_seqlen=77", "networks/dropout=dropout0",
                   "optimizer.config.fused=true", f"networks.image_encoder.micro_batch={args.micro_batch}", "networks.image_encoder.image_size=1024",
                   "+networks/image_encoder/augment=mammo"])
    spec = A.make_spec(cfg.networks.image_encoder.augment)
    seeding(cfg.base.seed)
    model = MMGCLIP(cfg).train()
    criterion = create_loss(cfg.loss.config.loss_name)()
    batch = synthetic_batch(args.batch, S=77, image_size=1024, seed=42)
    batch["text_tokens"] = batch["text_tokens"].to(dev)
    pix = {"fp32": batch["image"], "u16": as_pixel_dtype(batch["image"], "uint16")}
    pinned = True
    try:
        pix = {k: v.pin_memory() for k, v in pix.items()}
    except RuntimeError:
        pinned = False
    variants = {"fp32": ("fp32", None), "u16": ("u16", None), "u16_aug": ("u16", spec)}
    optimizer = None

    def step(kind, aug):
        nonlocal optimizer
        model.image_encoder.set_augment(aug)
        if optimizer is not None:
            optimizer.zero_grad(set_to_none=True)
        loss, _ = criterion(**model({**batch, "image": pix[kind]}, materialize_logits=False))      # (the model copies the pixels to the device)
        loss.backward()
        model.join_streams()
        if optimizer is None:
            optimizer = FusedAdamW(model.parameters(), lr=cfg.optimizer.config.learning_rate, weight_decay=cfg.optimizer.config.weight_decay)
        optimizer.step()
        return loss

    for kind, aug in variants.values():
        step(kind, aug)
    torch.cuda.synchronize()
    times, copies = {k: [] for k in variants}, {k: [] for k in pix}
    for _ in range(args.step_rounds):
        for k, (kind, aug) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = step(kind, aug)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
        for k, v in pix.items():                             # the host-to-device copy of the batch alone
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = v.to(dev)
            torch.cuda.synchronize()
            copies[k].append((time.perf_counter() - t0) * 1e3)
            del d
    assert torch.isfinite(loss)
    what = {"fp32": "fp32 pixels", "u16": "uint16 pixels", "u16_aug": "uint16 pixels + hflip 0.5, shift <= 32, gain [0.9, 1.1], offset [-0.05, 0.05]"}
    lines.extend(["## (b) the step", "",
                  f"C2 shape: ConvNeXt-T on [{args.batch}, 1, 1024, 1024] + BERT-base at S = 77, micro-batches of {args.micro_batch}, forward + backward + "
                  f"FusedAdamW; the pixels start on the host ({'pinned' if pinned else 'pageable'}) and are copied inside the timed step.  Host clock around "
                  f"a step that ends in a device synchronise; one warm-up step of every variant, then {args.step_rounds} rounds, alternating.", "",
                  "| variant | ms per step (each round) | median | pairs/s |", "|---|---|---|---|"])
    for k in variants:
        lines.append(f"| {what[k]} | {', '.join(f'{x:.1f}' for x in times[k])} | {med(times[k]):.1f} | {args.batch / med(times[k]) * 1e3:.0f} |")
    lines.extend(["", "The copy alone, same rounds: " + "; ".join(
        f"{k} {v.numel() * v.element_size() / 2 ** 30:.2f} GiB in {med(copies[k]):.1f} ms ({v.numel() * v.element_size() / med(copies[k]) / 1e6:.1f} GB/s)"
        for k, v in pix.items()) + ".", ""])


if args.part in ("kernel", "all"):
    kernel_part()
if args.part in ("step", "all"):
    step_part()
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
