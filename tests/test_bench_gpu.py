"""bench.py's plain run on one GPU, as the driver runs it: exactly --steps timed steps, ONE line without the --full legs, and with
--dump-outputs the last timed step's outputs as float32 .npy files - the same inputs, hence the same outputs, run after run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import measured

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"loss", "image_embeddings", "text_embeddings", "logit_scale", "param_sample", "grad_sample"}


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8",
           "--image-size", "224", "--micro-batch", "8", "--dump-outputs", out_dir]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    files = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}
    return json.loads(lines[0]), files


def test_plain_run_times_the_steps_and_dumps_the_last_one(dev, tmp_path):
    d, out = _plain_run(str(tmp_path / "a"))
    assert (d["n_gpus"], d["steps"], d["warmup"], d["higher_is_better"], d["dtype"]) == (1, 2, 1, True, "bf16")
    assert d["value"] > 0 and abs(d["value"] - 8 * 1000.0 / d["ms_per_step"]) < 0.02 * d["value"]
    for k in ("roofline", "next_kernels", "roofline_method", "cpu_baseline", "detail"):
        assert k not in d, k
    assert set(out) == NAMES
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert out["loss"].shape == () and abs(float(out["loss"]) - d["config"]["final_loss"]) < 1e-4
    for k in ("image_embeddings", "text_embeddings"):
        assert out[k].shape == (8, 512) and np.allclose(np.linalg.norm(out[k], axis=1), 1.0, atol=1e-3), k
    assert out["logit_scale"] == pytest.approx(1 / 0.07, rel=1e-2)
    assert out["param_sample"].size == out["grad_sample"].size > 10 ** 6 and np.abs(out["grad_sample"]).max() > 0

    # the same inputs again: what differs between two runs is only the order of the fp32 sums of the towers' weight-gradient atomics,
    # which three AdamW steps on 8 pairs carry into the loss at the 1e-3 level (0.18442 / 0.18477 in one pair of runs)
    d2, out2 = _plain_run(str(tmp_path / "b"))
    l1, l2 = d["config"]["final_loss"], d2["config"]["final_loss"]
    cos = {}
    for k in NAMES - {"loss", "logit_scale"}:
        a, b = out[k].ravel().astype(np.float64), out2[k].ravel().astype(np.float64)
        cos[k] = float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
    measured("bench_dump_run_to_run", loss_rel=abs(l2 - l1) / abs(l1), **{k + "_cos": v for k, v in cos.items()})
    assert abs(l2 - l1) < 1e-2 * abs(l1), (l1, l2)
    for k, c in cos.items():
        assert c > 0.999, (k, c)
