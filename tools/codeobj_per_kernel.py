#!/usr/bin/env python3
"""Per-kernel comparison of two gfx950 code objects, by symbol name: the instruction encodings of every kernel up to its last s_endpgm
(what follows is alignment padding, which depends on the neighbour) and the kernel's metadata entry (registers, LDS, kernarg layout).
For refactors that must leave the device code alone while the order in which kernels are emitted may change.  No GPU needed.

    llvm-objcopy --dump-section .hip_fatbin=x.fatbin x.o
    clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=x.fatbin --output=x.co
    tools/codeobj_per_kernel.py before.co after.co          (exit status 1 when a kernel differs)"""
import re, subprocess, sys, hashlib
import os
L = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "")
def kernels(co):
    out = subprocess.run([L + "llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    ks, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1); ks[cur] = []
        elif cur is not None and "//" in line:
            text, enc = line.split("//")
            ks[cur].append((text.split()[0], text.strip(), enc.split(":", 1)[1].strip()))
    for k, v in ks.items():
        last = max(i for i, t in enumerate(v) if t[0] == "s_endpgm")
        ks[k] = [t[1] + " | " + t[2] for t in v[:last + 1]]
    return ks
def metadata(co):
    out = subprocess.run([L + "llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    body = out[out.index("amdhsa.kernels:"):out.index("amdhsa.target:")]
    md = {}
    for block in re.split(r"\n  - ", body)[1:]:
        name = re.search(r"\.symbol:\s+(\S+)\.kd", block).group(1)
        md[name] = block.strip()
    return md
a, b, ma, mb = kernels(sys.argv[1]), kernels(sys.argv[2]), metadata(sys.argv[1]), metadata(sys.argv[2])
print(f"{sys.argv[1]} vs {sys.argv[2]}: {len(a)} / {len(b)} kernels,", "same names" if sorted(a) == sorted(b) == sorted(ma) == sorted(mb) else "NAMES DIFFER")
bad = 0
for k in sorted(a):
    same, msame = a[k] == b.get(k), ma[k] == mb.get(k)
    bad += not (same and msame)
    print("code", "same" if same else "DIFF", " metadata", "same" if msame else "DIFF", f"{len(a[k]):5d} instructions", hashlib.sha256("\n".join(a[k]).encode()).hexdigest()[:16], k)
sys.exit(bad != 0)
