"""Param groups for the fine-tuning recipe, everything that needs no GPU: the pure group builder (optim_groups.py), the config surface,
construction of both optimizers from the same groups, the schedulers over several groups, the chunk-map builder on a host arena and
the argument validation of mmg_adamw_step_groups (before any HIP call)."""
import ctypes
import math
import os

import pytest
import torch

from tests.test_grad_clip_cpu import _host_experiment
from tests.test_grad_clip_gpu import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "mmg-clip_amd", "configs")
LR, WD = 5e-5, 1e-4


class _Clip(torch.nn.Module):
    """MMGCLIP's parameter layout around real towers (built on the host: parameters only, nothing runs)."""

    def __init__(self, image, text):
        super().__init__()
        self.image_encoder, self.text_encoder = image, text
        self.image_projection_layer = torch.nn.Linear(8, 4, bias=False)
        self.text_projection_layer = torch.nn.Linear(8, 4, bias=False)
        self.logit_scale = torch.nn.Parameter(torch.tensor(2.6593))


def _convnext():
    from mmgclip.networks.encoder import ConvNextTinyEncoder
    return ConvNextTinyEncoder()


def _bert(layers=2):
    from mmgclip.networks.bert import BertConfigLite
    from mmgclip.networks.encoder import BertEncoder
    return BertEncoder(random_init=True, freeze=True, config=BertConfigLite(num_hidden_layers=layers, vocab_size=300))


def _vit(layers=2):
    from mmgclip.networks.encoder import ViTB16Encoder
    return ViTB16Encoder(image_size=32, layers=layers)


def _by_name(model, groups):
    """{full parameter name: its group}; asserts that every parameter sits in exactly one group."""
    names = {id(p): n for n, p in model.named_parameters()}
    seen = {}
    for g in groups:
        assert set(g) == {"params", "lr", "weight_decay", "name"}
        for p in g["params"]:
            assert names[id(p)] not in seen, names[id(p)]
            seen[names[id(p)]] = g
    assert set(seen) == set(names.values())
    return seen


def _ordered_by_first_appearance(model, groups):
    order = {id(p): i for i, p in enumerate(model.parameters())}
    firsts = [min(order[id(p)] for p in g["params"]) for g in groups]
    inside = all([order[id(p)] for p in g["params"]] == sorted(order[id(p)] for p in g["params"]) for g in groups)
    return firsts == sorted(firsts) and inside


# ---- defaults ----------------------------------------------------------------------------------------------------------------------
def test_defaults_build_the_one_group_of_today(tmp_path, monkeypatch):
    from mmgclip.optim_groups import build_param_groups
    model = _Clip(_convnext(), _bert())
    groups = build_param_groups(model, LR, WD)
    assert len(groups) == 1 and groups[0]["lr"] == LR and groups[0]["weight_decay"] == WD
    assert len(groups[0]["params"]) == len(list(model.parameters()))
    assert all(a is b for a, b in zip(groups[0]["params"], model.parameters()))
    for fused in ("true", "false"):
        exp = _host_experiment(tmp_path, [f"optimizer.config.fused={fused}"], [], monkeypatch)
        assert len(exp.optimizer.param_groups) == 1 and "name" not in exp.optimizer.param_groups[0]
        assert all(a is b for a, b in zip(exp.optimizer.param_groups[0]["params"], exp.model.parameters()))
        assert exp.optimizer.param_groups[0]["weight_decay"] == exp.config.optimizer.config.weight_decay


# ---- layer ids and scales ------------------------------------------------------------------------------------------------------------
def test_convnext_tiny_bert_layer_ids_scales_and_no_decay_set():
    from mmgclip.optim_groups import build_param_groups, is_no_decay, layer_ids
    model = _Clip(_convnext(), _bert(2))
    rel = [n for n, _ in model.image_encoder.model.named_parameters()]
    ids, B = layer_ids(rel)
    assert B == 18 and ids["features.0.0.weight"] == 0 and ids["features.0.1.bias"] == 0
    assert ids["features.1.0.layer_scale"] == 1 and ids["features.1.2.block.0.weight"] == 3
    assert ids["features.2.1.weight"] == ids["features.3.0.block.0.weight"] == 4
    assert ids["features.4.0.weight"] == ids["features.5.0.layer_scale"] == 7
    assert ids["features.5.8.block.3.weight"] == 15 and ids["features.6.1.bias"] == 16 and ids["features.7.2.block.5.bias"] == 18
    assert sorted(set(ids.values())) == list(range(19))
    tids, L = layer_ids([n for n, _ in model.text_encoder.model.named_parameters()])
    assert L == 2 and tids["embeddings.word_embeddings.weight"] == 0 and tids["embeddings.LayerNorm.bias"] == 0
    assert tids["encoder.layer.0.attention.self.query.weight"] == 1 and tids["encoder.layer.1.output.LayerNorm.weight"] == 2
    assert tids["pooler.dense.weight"] == 2

    d = 0.75
    groups = build_param_groups(model, LR, WD, layer_decay=d, no_decay_1d=True, image_lr_mult=2.0, text_lr_mult=0.5)
    by = _by_name(model, groups)                                     # every parameter exactly once (the frozen BERT included)
    assert _ordered_by_first_appearance(model, groups)
    assert len({g["name"] for g in groups}) == len(groups)
    for n, p in model.named_parameters():
        g = by[n]
        if n.startswith("image_encoder.model."):
            want = LR * 2.0 * d ** (18 - ids[n[len("image_encoder.model."):]])
        elif n.startswith("text_encoder.model."):
            want = LR * 0.5 * d ** (2 - tids[n[len("text_encoder.model."):]])
        else:
            want = LR                                                # heads and logit_scale: scale 1
        assert math.isclose(g["lr"], want, rel_tol=1e-12), (n, g["lr"], want)
        rule = p.ndim <= 1 or n.endswith("layer_scale") or n.endswith("class_token") or n.endswith("encoder.pos_embedding")
        assert is_no_decay(n, p) == rule
        assert g["weight_decay"] == (0.0 if rule else WD), n
    assert by["image_encoder.model.features.7.2.block.3.weight"]["lr"] == LR * 2.0          # the last block: scale exactly 1
    assert by["text_encoder.model.pooler.dense.weight"]["lr"] == LR * 0.5
    assert by["image_encoder.model.features.1.0.layer_scale"]["weight_decay"] == 0.0          # [C,1,1], by name
    assert by["logit_scale"]["weight_decay"] == 0.0 and by["logit_scale"]["lr"] == LR          # 0-d
    assert by["image_encoder.model.features.0.0.weight"]["weight_decay"] == WD                # stem conv
    assert by["image_encoder.model.features.1.0.block.0.weight"]["weight_decay"] == WD        # depthwise conv
    assert by["image_encoder.model.features.1.0.block.0.bias"]["weight_decay"] == 0.0
    assert by["image_projection_layer.weight"]["weight_decay"] == WD and by["image_projection_layer.weight"]["lr"] == LR
    # the same groups from a second model of the same architecture: a function of names and shapes alone
    other = build_param_groups(_Clip(_convnext(), _bert(2)), LR, WD, layer_decay=d, no_decay_1d=True, image_lr_mult=2.0, text_lr_mult=0.5)
    assert [(g["name"], g["lr"], g["weight_decay"], [tuple(p.shape) for p in g["params"]]) for g in other] == \
           [(g["name"], g["lr"], g["weight_decay"], [tuple(p.shape) for p in g["params"]]) for g in groups]


def test_vit_layer_ids_and_no_decay_set():
    from mmgclip.optim_groups import build_param_groups, layer_ids
    model = _Clip(_vit(2), _bert(2))
    ids, L = layer_ids([n for n, _ in model.image_encoder.model.named_parameters()])
    assert L == 2 and ids["conv_proj.weight"] == ids["class_token"] == ids["encoder.pos_embedding"] == 0
    assert ids["encoder.layers.encoder_layer_0.ln_1.weight"] == 1 and ids["encoder.layers.encoder_layer_1.mlp.3.bias"] == 2
    assert ids["encoder.ln.weight"] == 2
    groups = build_param_groups(model, LR, WD, layer_decay=0.5, no_decay_1d=True)
    by = _by_name(model, groups)
    assert _ordered_by_first_appearance(model, groups)
    pre = "image_encoder.model."
    assert by[pre + "class_token"]["weight_decay"] == 0.0 and by[pre + "encoder.pos_embedding"]["weight_decay"] == 0.0
    assert by[pre + "conv_proj.weight"]["weight_decay"] == WD and by[pre + "conv_proj.weight"]["lr"] == LR * 0.25
    assert by[pre + "encoder.layers.encoder_layer_0.self_attention.in_proj_weight"]["lr"] == LR * 0.5
    assert by[pre + "encoder.ln.bias"]["lr"] == LR and by[pre + "encoder.layers.encoder_layer_1.mlp.0.weight"]["lr"] == LR
    assert by["logit_scale"]["lr"] == LR and by["text_projection_layer.weight"]["lr"] == LR
    # no_decay_1d alone: two kinds of weight decay, no learning rate but lr
    plain = build_param_groups(model, LR, WD, no_decay_1d=True)
    assert {g["lr"] for g in plain} == {LR} and {g["weight_decay"] for g in plain} == {0.0, WD}


def test_bad_values_raise():
    from mmgclip.optim_groups import build_param_groups
    model = torch.nn.Linear(3, 2)
    for bad in (0, 0.0, -0.5, 1.5, float("nan"), float("inf"), "0.5", True):
        with pytest.raises(ValueError, match="layer_decay"):
            build_param_groups(model, LR, WD, layer_decay=bad)
    for key in ("image_lr_mult", "text_lr_mult"):
        for bad in (0, -1.0, float("nan"), float("inf"), None, "2"):
            with pytest.raises(ValueError, match=key):
                build_param_groups(model, LR, WD, **{key: bad})
    assert len(build_param_groups(model, LR, WD, layer_decay=1.0, image_lr_mult=2, text_lr_mult=0.1)) == 1     # no tower: all heads


# ---- the config surface and both optimizers --------------------------------------------------------------------------------------------
def test_finetune_config_and_overrides_reach_both_optimizers(tmp_path, monkeypatch):
    from mmgclip.config import compose
    from mmgclip.optim import FusedAdamW
    c = compose(CFG_DIR, "train_binary_class_clf", ["optimizer=adamw_finetune"])
    oc = c.optimizer.config
    assert (oc.fused, oc.layer_decay, oc.no_decay_1d, oc.max_grad_norm, oc.learning_rate, oc.weight_decay) == (True, 0.75, True, 1.0, 5e-5, 1e-4)
    shipped = compose(CFG_DIR, "train_binary_class_clf").optimizer.config
    assert (shipped.learning_rate, shipped.weight_decay) == (oc.learning_rate, oc.weight_decay)       # the reference's

    def layout(exp):
        names = {id(p): n for n, p in exp.model.named_parameters()}
        return [(g["name"], g["lr"], g["initial_lr"], g["weight_decay"], [names[id(p)] for p in g["params"]]) for g in exp.optimizer.param_groups]
    fused = _host_experiment(tmp_path, ["optimizer=adamw_finetune"], [], monkeypatch)
    plain = _host_experiment(tmp_path, ["optimizer=adamw_finetune", "optimizer.config.fused=false"], [], monkeypatch)
    assert isinstance(fused.optimizer, FusedAdamW) and fused.optimizer.max_grad_norm == 1.0 and type(plain.optimizer).__name__ == "AdamW"
    assert layout(fused) == layout(plain) and len(fused.optimizer.param_groups) == 2          # the stand-in: two weights, and logit_scale without decay
    assert {g["weight_decay"] for g in fused.optimizer.param_groups} == {0.0, 1e-4}
    # the four keys as overrides on the shipped optimizer config (the stand-in has no towers: the multipliers and the decay find nothing)
    over = ["optimizer.config.layer_decay=0.9", "optimizer.config.no_decay_1d=true", "optimizer.config.image_lr_mult=0.5",
            "optimizer.config.text_lr_mult=2.0"]
    a = _host_experiment(tmp_path, over + ["optimizer.config.fused=true"], [], monkeypatch)
    b = _host_experiment(tmp_path, over, [], monkeypatch)
    assert isinstance(a.optimizer, FusedAdamW) and type(b.optimizer).__name__ == "AdamW" and layout(a) == layout(b) and len(layout(a)) == 2
    for bad in ("optimizer.config.layer_decay=1.5", "optimizer.config.layer_decay=0", "optimizer.config.text_lr_mult=-1",
                "optimizer.config.image_lr_mult=0"):
        with pytest.raises(ValueError):
            _host_experiment(tmp_path, [bad], [], monkeypatch)


def test_real_towers_reach_both_optimizers_as_the_same_groups():
    """build_param_groups over ConvNeXt-T + BERT -> FusedAdamW and torch.optim.AdamW: the same param_groups, every key of them."""
    from mmgclip.optim import FusedAdamW
    from mmgclip.optim_groups import build_param_groups
    model = _Clip(_convnext(), _bert(2))
    groups = build_param_groups(model, LR, WD, layer_decay=0.75, no_decay_1d=True)
    a, b = FusedAdamW(groups, lr=LR, weight_decay=WD), torch.optim.AdamW(groups, lr=LR, weight_decay=WD)
    assert len(a.param_groups) == len(b.param_groups) == len(groups) > 20
    for ga, gb in zip(a.param_groups, b.param_groups):
        assert (ga["name"], ga["lr"], ga["weight_decay"], ga["betas"], ga["eps"]) == (gb["name"], gb["lr"], gb["weight_decay"], gb["betas"], gb["eps"])
        assert all(x is y for x, y in zip(ga["params"], gb["params"]))


# ---- schedulers -------------------------------------------------------------------------------------------------------------------------
def test_schedulers_keep_the_ratios_between_groups():
    from mmgclip.scheduler.warmup_cosine import LinearWarmupCosineAnnealingLR
    ws = [torch.nn.Parameter(torch.zeros(2)) for _ in range(3)]
    base = [5e-5, 5e-5 * 0.75, 5e-5 * 0.75 ** 7]

    def groups():
        return [dict(params=[w], lr=lr, weight_decay=1e-4, name=str(i)) for i, (w, lr) in enumerate(zip(ws, base))]
    opt = torch.optim.AdamW(groups(), lr=1.0)
    sch = LinearWarmupCosineAnnealingLR(opt, total_steps=15, warmup_steps=2)
    seen = set()
    for _ in range(6):
        opt.step()
        sch.step()
        lrs = [g["lr"] for g in opt.param_groups]
        assert lrs[0] > 0
        seen.add(lrs[0])
        for lr, b in zip(lrs, base):
            assert math.isclose(lr / lrs[0], b / base[0], rel_tol=1e-12)
    assert len(seen) > 3                                             # the schedule really moved
    opt = torch.optim.AdamW(groups(), lr=1.0)
    plateau = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, "min", patience=0)
    for _ in range(3):
        plateau.step(1.0)
    lrs = [g["lr"] for g in opt.param_groups]
    assert lrs[0] < base[0]                                          # it reduced
    for lr, b in zip(lrs, base):
        assert math.isclose(lr / lrs[0], b / base[0], rel_tol=1e-12)


# ---- the chunk map ----------------------------------------------------------------------------------------------------------------------
def test_chunk_map_on_a_host_arena():
    from mmgclip.optim import build_chunk_map
    from mmgclip.params import ParamArena
    g = torch.Generator().manual_seed(0)
    arena = ParamArena([(f"w{i}", torch.nn.Parameter(torch.randn(s, generator=g))) for i, s in enumerate(SHAPES)], torch.device("cpu"))
    assert len(SHAPES) == 20
    slots = [i % 2 for i in range(len(SHAPES))]                     # groups alternating tensor by tensor
    cmap = build_chunk_map(arena, slots)
    assert cmap.dtype == torch.uint8 and cmap.numel() == arena.size // 64 and arena.size % 64 == 0
    covered = 0
    for n, p, s in zip(arena.names, arena.params, slots):
        first, count = arena.offsets[n] // 64, (p.numel() + 63) // 64
        assert arena.offsets[n] % 64 == 0 and bool((cmap[first:first + count] == s).all())
        covered += count
    assert covered == cmap.numel()                                  # every chunk belongs to exactly one parameter
    three = build_chunk_map(arena, [i % 3 for i in range(len(SHAPES))])
    assert sorted(set(three.tolist())) == [0, 1, 2]


# ---- the entry point's argument checks --------------------------------------------------------------------------------------------------
def test_adamw_step_groups_rejects_bad_arguments_without_a_gpu():
    """Validation happens before any HIP call: the device pointers are stand-ins and are never dereferenced."""
    from mmgclip import _hip
    lib = _hip.load()
    assert lib.mmg_abi_version() == 5
    d = 0x1000
    lr, wd = (ctypes.c_float * 129)(*([1e-3] * 129)), (ctypes.c_float * 129)(*([0.0] * 129))
    ok = [d, d, d, d, 128, d, 2, lr, wd, 0.9, 0.999, 1e-8, 1, None, None, None]

    def rejected(**change):
        args = list(ok)
        for i, val in change.items():
            args[int(i[1:])] = val
        rc = lib.mmg_adamw_step_groups(*args)
        return rc != 0 and b"mmg_adamw_step_groups" in lib.mmg_last_error()
    for i in (0, 1, 2, 3, 5, 7, 8):                                  # p, g, m, v, chunk_group, group_lr, group_wd
        assert rejected(**{f"a{i}": None}), i
        assert b"null" in lib.mmg_last_error()
    assert rejected(a4=100) and b"multiple of 64" in lib.mmg_last_error()
    assert rejected(a4=0) and rejected(a4=-64) and rejected(a12=0)
    assert rejected(a6=0) and b"n_groups" in lib.mmg_last_error()
    assert rejected(a6=129) and b"n_groups" in lib.mmg_last_error()
    for i in (0, 1, 2, 3):
        assert rejected(**{f"a{i}": d + 4}) and b"aligned" in lib.mmg_last_error()
    assert rejected(a14=d) and b"skipped" in lib.mmg_last_error()    # skipped without clip
