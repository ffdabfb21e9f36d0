"""Gradient clipping by global norm / the non-finite-step guard: everything that needs no GPU - the config surface, the optimizer's
argument checks, the entry points' argument validation (before any HIP call) and the torch.optim.AdamW (`fused: false`) path of
`ClassifierExperiment.train()` on the host stand-in model of tests/test_distributed_cpu.py."""
import os

import pytest
import torch

from tests.test_distributed_cpu import OracleHeadBackend, _OracleClipLoss, _TinyClip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "mmg-clip_amd", "configs")


def test_shipped_configs_compose_with_the_guard_off():
    from mmgclip.config import compose, overridden_keys
    for name in ("train_binary_class_clf", "train_exam_reports_clf"):
        c = compose(CFG_DIR, name)
        assert c.optimizer.config.max_grad_norm is None and c.optimizer.config.skip_nonfinite is True
        assert "optimizer.config.skip_nonfinite" not in overridden_keys(c)
    c = compose(CFG_DIR, "train_binary_class_clf", ["optimizer=adamw_decay1e-2", "optimizer.config.max_grad_norm=0.5"])
    assert c.optimizer.config.max_grad_norm == 0.5 and c.optimizer.config.weight_decay == 1e-2
    assert "optimizer.config.max_grad_norm" in overridden_keys(c)


def _host_experiment(tmp, overrides, loader, monkeypatch):
    """The experiment on the host: the two-linear-layer stand-in for MMGCLIP, the oracle head behind the product loss."""
    from mmgclip import head
    from mmgclip.config import compose
    from mmgclip.experiments import ClassifierExperiment as CE
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(head, "_HipHeadBackend", OracleHeadBackend)
    monkeypatch.setattr(CE, "model", _TinyClip)
    cfg = compose(CFG_DIR, "train_binary_class_clf", [f"checkpoints.checkpoints_export_dir={tmp}", f"base.tensorboard_export_dir={tmp}",
                                                      "optimizer.config.learning_rate=0.05"] + list(overrides))
    exp = CE.ClassifierExperiment(config=cfg, train_dataloader=loader, valid_dataloader=None, test_dataloader=None, tokenizer=None)
    exp.criterion = _OracleClipLoss(None)
    return exp


def test_override_reaches_the_fused_optimizer(tmp_path, monkeypatch):
    """Construction only: `max_grad_norm=0.5` with `fused: true` arrives in FusedAdamW; a shipped config leaves it unguarded; an
    explicit `skip_nonfinite=true` without a norm guards without clipping."""
    from mmgclip.optim import FusedAdamW
    exp = _host_experiment(tmp_path, ["optimizer.config.fused=true", "optimizer.config.max_grad_norm=0.5"], [], monkeypatch)
    assert isinstance(exp.optimizer, FusedAdamW) and exp.optimizer.max_grad_norm == 0.5 and exp.optimizer.skip_nonfinite is True
    exp = _host_experiment(tmp_path, ["optimizer.config.fused=true", "optimizer.config.max_grad_norm=0.5",
                                      "optimizer.config.skip_nonfinite=false"], [], monkeypatch)
    assert exp.optimizer.max_grad_norm == 0.5 and exp.optimizer.skip_nonfinite is False
    exp = _host_experiment(tmp_path, ["optimizer.config.fused=true"], [], monkeypatch)
    assert exp.optimizer.max_grad_norm is None and exp.optimizer.skip_nonfinite is False
    assert exp.optimizer.grad_norm is None and exp.optimizer.skipped_steps() == 0
    exp = _host_experiment(tmp_path, ["optimizer.config.fused=true", "optimizer.config.skip_nonfinite=true"], [], monkeypatch)
    assert exp.optimizer.max_grad_norm is None and exp.optimizer.skip_nonfinite is True


def test_fused_adamw_rejects_a_bad_max_grad_norm():
    from mmgclip.optim import FusedAdamW
    p = torch.nn.Parameter(torch.zeros(3))
    for bad in (-1, -1.0, 0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdamW([p], max_grad_norm=bad)
    opt = FusedAdamW([p])                                   # the default: the unguarded step
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False
    opt = FusedAdamW([p], max_grad_norm=2)
    assert opt.max_grad_norm == 2.0 and opt.skip_nonfinite is True
    assert FusedAdamW([p], skip_nonfinite=True).skip_nonfinite is True


def test_partials_count_is_a_function_of_n_alone():
    from mmgclip import _hip
    lib = _hip.load()
    assert lib.mmg_grad_sumsq_partials(1) == 1 and lib.mmg_grad_sumsq_partials(8192) == 1 and lib.mmg_grad_sumsq_partials(8193) == 2
    assert lib.mmg_grad_sumsq_partials(1 << 24) == 2048 and lib.mmg_grad_sumsq_partials((1 << 24) + 5) == 2048
    assert lib.mmg_grad_sumsq_partials(1 << 40) == 2048                     # capped
    assert lib.mmg_grad_sumsq_partials(0) == 0 and lib.mmg_grad_sumsq_partials(-3) == 0


def test_bad_arguments_are_rejected_without_a_gpu():
    """Argument validation happens before any HIP call (the pointers are never dereferenced on the host)."""
    from mmgclip import _hip
    lib = _hip.load()
    g, part = 0x1000, 0x2000                                # stand-in device addresses
    assert lib.mmg_grad_sumsq(None, 16, part, 1, None) != 0 and b"mmg_grad_sumsq" in lib.mmg_last_error()
    assert lib.mmg_grad_sumsq(g, 16, None, 1, None) != 0
    assert lib.mmg_grad_sumsq(g, 0, part, 0, None) != 0 and lib.mmg_grad_sumsq(g, -5, part, 1, None) != 0
    assert lib.mmg_grad_sumsq(g, 8193, part, 1, None) != 0 and b"n_partials" in lib.mmg_last_error()        # takes 2
    assert lib.mmg_grad_sumsq(g, 16, part, 2, None) != 0 and b"n_partials" in lib.mmg_last_error()          # takes 1
    assert lib.mmg_grad_sumsq(g + 2, 16, part, 1, None) != 0 and b"aligned" in lib.mmg_last_error()
    assert lib.mmg_grad_clip_finalize(None, 4, 1.0, g, None, None) != 0 and b"mmg_grad_clip_finalize" in lib.mmg_last_error()
    assert lib.mmg_grad_clip_finalize(part, 4, 1.0, None, None, None) != 0
    assert lib.mmg_grad_clip_finalize(part, 0, 1.0, g, None, None) != 0
    assert lib.mmg_grad_clip_finalize(part, 4, float("nan"), g, None, None) != 0 and b"NaN" in lib.mmg_last_error()
    ok = (g, g, g, g, None, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, g, None, None)
    for i in (0, 1, 2, 3, 12):                              # p, g, m, v, clip
        bad = list(ok)
        bad[i] = None
        assert lib.mmg_adamw_step_guarded(*bad) != 0 and b"mmg_adamw_step_guarded" in lib.mmg_last_error()
    for i, val in ((5, 0), (5, -1), (11, 0)):               # n <= 0, step < 1
        bad = list(ok)
        bad[i] = val
        assert lib.mmg_adamw_step_guarded(*bad) != 0


# ---- `fused: false`: torch.nn.utils.clip_grad_norm_ between the backward and torch.optim.AdamW's step ----------------------------
def _batches(steps=3, n=8, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [{"image_features": torch.randn(n, 16, generator=g), "text": torch.randn(n, 16, generator=g)} for _ in range(steps)]


def test_unfused_train_epoch_equals_a_hand_written_clipped_loop(tmp_path, monkeypatch):
    max_norm = 0.05
    exp = _host_experiment(tmp_path, [f"optimizer.config.max_grad_norm={max_norm}"], _batches(), monkeypatch)
    assert type(exp.optimizer).__name__ == "AdamW"
    exp.scheduler.step()                                    # leave the reference's lr-0 first epoch
    # the same model, optimizer and schedule by hand
    ref = _TinyClip()
    opt = torch.optim.AdamW(ref.parameters(), lr=0.05, weight_decay=exp.config.optimizer.config.weight_decay)
    for g in opt.param_groups:
        g["lr"] = exp.optimizer.param_groups[0]["lr"]
    crit = _OracleClipLoss(None)
    norms = []
    for b in _batches():
        opt.zero_grad(set_to_none=True)
        loss, _ = crit(**ref(b))
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)))
        opt.step()
    assert min(norms) > 2 * max_norm, norms                 # the bound binds at every step
    exp.train()
    for (k, a), (_, b) in zip(exp.model.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k
    assert exp.skipped_steps == 0 and float(exp._last_grad_norm) == norms[-1]
    # and it is not the unclipped trajectory
    free = _host_experiment(tmp_path, [], _batches(), monkeypatch)
    free.scheduler.step()
    free.train()
    assert not torch.equal(free.model.state_dict()["text_encoder.weight"], exp.model.state_dict()["text_encoder.weight"])


def test_unfused_nan_loss_leaves_every_parameter_unchanged(tmp_path, monkeypatch):
    bad = _batches(1)
    bad[0]["text"][3, 5] = float("nan")
    exp = _host_experiment(tmp_path, ["optimizer.config.max_grad_norm=1.0"], bad, monkeypatch)
    exp.scheduler.step()
    before = {k: v.clone() for k, v in exp.model.state_dict().items()}
    loss = exp.train()
    assert loss != loss                                     # the batch really gave a NaN loss
    for k, v in exp.model.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert exp.skipped_steps == 1 and len(exp.optimizer.state) == 0


def test_host_powf_against_fp64_repeated_squaring():
    """The unguarded step takes beta^t from the host's powf, the guarded kernel forms it by repeated squaring in fp64 and rounds to fp32
    (csrc/grad_clip.hip: pow_int, restated here).  beta^1 is beta on both sides; elsewhere the two may differ, by one fp32 ulp at most.
    Prints how often they do on this libm (DESIGN.md section 4 quotes the counts)."""
    import ctypes
    import ctypes.util

    import numpy as np
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]

    def pow_int(beta, t):
        b, r = float(np.float32(beta)), 1.0
        while t > 0:
            if t & 1:
                r *= b
            b *= b
            t >>= 1
        return np.float32(r)
    for beta in (0.9, 0.999):
        assert np.float32(libm.powf(beta, 1.0)) == pow_int(beta, 1) == np.float32(beta)
        differ = []
        for t in range(1, 20001):
            h, d = np.float32(libm.powf(beta, float(t))), pow_int(beta, t)
            if h != d:
                differ.append(t)
                assert abs(float(h) - float(d)) <= float(np.spacing(d)) * 1.0000001, (beta, t, h, d)
        print(f"beta {beta}: host powf != fp64 repeated squaring at {len(differ)} of 20000 values of t, first {differ[:3]}")
        assert len(differ) < 400            # rare: powf is within one ulp and mostly correctly rounded
