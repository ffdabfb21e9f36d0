#!/usr/bin/env python3
"""Timing ablations of the matrix-core depthwise kernel (csrc/dwconv7_mfma.hip): which phase of an item costs what?

The phase mask is a BUILD constant (-DDWM_DBG=<mask>: 1 skip B, 2 skip D, 4 skip E, 8 skip F, 16 skip the global loads; results are then
wrong), not an environment knob: build one library per mask first, where hipcc is,

    for m in 1 2 4 8 16 3 7 15 31 24; do tools/build_ab_lib.sh dwm$m dwconv7_mfma -DDWM_DBG=$m; done

then run `tools/dwm_ablate.py` on the GPU box: it times the product library (mask 0) and every tools/libmmg_ab_dwm<mask>.so it finds,
each in a fresh child process (MMGCLIP_HIP_LIB selects the library when the package is first imported), two rounds."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: "everything", 1: "no B (transpose in)", 2: "no D (MFMA)", 4: "no E (transpose out)", 8: "no F (stores)", 16: "no global loads",
         3: "no B, D", 7: "no B, D, E", 15: "no B, D, E, F", 31: "nothing but deposit + barriers", 24: "no loads, no stores"}


def timeit(iters=10):
    sys.path.insert(0, os.path.join(ROOT, "mmg-clip_amd"))
    import torch
    from mmgclip import kernels as K
    dev = torch.device("cuda:0")
    n, H, C = 16, 256, 96
    x = torch.randn(n * H * H, C, device=dev).bfloat16()
    w = torch.randn(49, C, device=dev) * 0.1
    b = torch.randn(C, device=dev)
    out = torch.empty_like(x)
    K.dwconv7(x, w, b, n, H, H, C, out=out); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        K.dwconv7(x, w, b, n, H, H, C, out=out)
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        print(f"{timeit():8.1f} us", flush=True)
        sys.exit(0)
    libs = {m: os.path.join(ROOT, "tools", f"libmmg_ab_dwm{m}.so") for m in NAMES if m}
    missing = [m for m, p in libs.items() if not os.path.isfile(p)]
    if missing:
        print("no library for the masks", missing, "- build them first: tools/build_ab_lib.sh dwm<mask> dwconv7_mfma -DDWM_DBG=<mask>")
    for rnd in range(2):
        for m, nm in NAMES.items():
            if m in missing:
                continue
            env = dict(os.environ, MMG_DWCONV_MFMA="1")
            if m:
                env["MMGCLIP_HIP_LIB"] = libs[m]
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=300)
            print(f"round {rnd}  dbg {m:2d}  {nm:32s} {r.stdout.strip() if r.returncode == 0 else 'FAILED: ' + r.stderr[-300:]}", flush=True)
            if r.returncode != 0:
                sys.exit(1)          # (a child that failed on the GPU: start nothing more on it)
