#!/usr/bin/env python3
"""What training the ConvNeXt-T tower at a mammogram's native size costs against padding it to the next multiple of 32: forward + backward of
the tower alone at n = 32, 1906 x 818 and at 1920 x 832 (HIP events, warm-up first), and which stage-1 backward path the micro-batch takes.

    python tools/native_size_cost.py [n] [reps]
"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
import torch                                                   # noqa: E402
from mmgclip import kernels as K                               # noqa: E402
from mmgclip.networks.encoder import ConvNextTinyEncoder       # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")
torch.manual_seed(0)
tower = ConvNextTinyEncoder(micro_batch=n).to(dev)
res = {}
for H, W in ((1906, 818), (1920, 832), (1906, 818), (1920, 832)):
    img = torch.rand(n, 1, H, W, device=dev)
    wgt = torch.randn(n, 768, device=dev)

    def step():
        tower.zero_grad(set_to_none=True)
        (tower(img) * wgt).sum().backward()
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        step()
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / reps
    h, w = H // 4, W // 4
    path = "cnblock_bwdw" if (tower.bwdw and K.cnblock_bwdw_supported(96, n * h * w)) else "cnblock_mlp_bwd + 2 weight-gradient GEMMs"
    res.setdefault((H, W), []).append(ms)
    print(f"n={n} {H}x{W}: stage-1 map {h}x{w} ({n * h * w} rows, stage-1 backward: {path}), last map {tower.feature_map_shape(H, W)}, "
          f"forward + backward {ms:.1f} ms, {H * W * n / ms / 1e6:.1f} Gpixel/s", flush=True)
    del img, wgt
a, b = min(res[(1906, 818)]), min(res[(1920, 832)])
print(f"native / padded = {a / b:.3f} (pixels: {1906 * 818 / (1920 * 832):.3f})")
