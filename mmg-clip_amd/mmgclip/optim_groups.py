"""torch param groups for the fine-tuning recipe: no weight decay on 1-d parameters, layer-wise learning-rate decay, a learning-rate
multiplier per tower.  The reference hands `model.parameters()` to torch.optim.AdamW as one group
(mmgclip/experiments/ClassifierExperiment.py:74), and with every option at its default so does `build_param_groups`.

Pure Python over parameter names and shapes: no GPU, no arena (the towers build theirs at their first forward, after the optimizer),
and the same groups on every data-parallel rank.  The groups go to `optim.FusedAdamW` and to `torch.optim.AdamW` alike; FusedAdamW
still updates a tower's arena in one launch (csrc/adamw_groups.hip).

Layer ids, read from the tower-relative names (the names the arenas use), k of L -> lr * mult * layer_decay ** (L - k):
  ConvNeXt  features.0.* -> 0; the blocks features.{1,3,5,7}.{j}.* -> 1 ... B in depth order; a downsample layer features.{2,4,6}.* -> the
            id of the first block it feeds; L = B
  BERT      embeddings.* -> 0; encoder.layer.{i}.* -> i + 1; pooler.* -> L = number of layers
  ViT       conv_proj.*, class_token, encoder.pos_embedding -> 0; encoder_layer_{i} -> i + 1; encoder.ln.* -> L = number of layers
  ResNet    none (only layer4 trains)
Projection heads, logit_scale and logit_bias (the sigmoid loss's) are no tower's: neither layer_decay nor a tower multiplier touches
them; the two 0-d scalars are in the no-decay set at the base learning rate."""
import math
import re

import torch.nn as nn

_CONVNEXT = re.compile(r"features\.(\d+)\.(\d+)\.")
_BERT = re.compile(r"encoder\.layer\.(\d+)\.")
_VIT = re.compile(r"encoder\.layers\.encoder_layer_(\d+)\.")


def _is_tower(mod):
    """networks.tower.Tower, by its surface: the parameters under `.model` are what goes into the arena."""
    return hasattr(mod, "_arena_parameters") and isinstance(getattr(mod, "model", None), nn.Module)


def tower_kind(names):
    """'convnext' / 'bert' / 'vit' from a tower's parameter names, None for anything else (ResNet: no layer ids)."""
    if any(_CONVNEXT.match(n) for n in names):
        return "convnext"
    if any(_BERT.match(n) for n in names):
        return "bert"
    if any(_VIT.match(n) for n in names):
        return "vit"
    return None


def layer_ids(names):
    """{name: layer id}, L for the tower-relative parameter names of one tower; ({}, 0) when the tower has no layer table."""
    kind = tower_kind(names)
    ids = {}
    if kind == "convnext":
        blocks = sorted({(int(m.group(1)), int(m.group(2))) for m in map(_CONVNEXT.match, names) if m and int(m.group(1)) % 2 == 1})
        number = {sj: k + 1 for k, sj in enumerate(blocks)}
        for n in names:
            stage = int(n.split(".")[1])
            if stage == 0:
                ids[n] = 0
            elif stage % 2 == 1:
                m = _CONVNEXT.match(n)
                ids[n] = number[(stage, int(m.group(2)))]
            else:
                ids[n] = number[(stage + 1, 0)]
        return ids, len(blocks)
    if kind == "bert":
        L = 1 + max(int(m.group(1)) for m in map(_BERT.match, names) if m)
        for n in names:
            m = _BERT.match(n)
            ids[n] = int(m.group(1)) + 1 if m else (0 if n.startswith("embeddings.") else L)
        return ids, L
    if kind == "vit":
        L = 1 + max(int(m.group(1)) for m in map(_VIT.match, names) if m)
        for n in names:
            m = _VIT.match(n)
            ids[n] = int(m.group(1)) + 1 if m else (L if n.startswith("encoder.ln.") else 0)
        return ids, L
    return {}, 0


def is_no_decay(name, param):
    """The parameters every published ConvNeXt / ViT / BERT recipe keeps out of weight decay."""
    return param.ndim <= 1 or name in ("logit_scale", "logit_bias") or name.endswith("layer_scale") or name.endswith("class_token") or name.endswith("encoder.pos_embedding")


def _check(layer_decay, mults):
    if layer_decay is not None and not (isinstance(layer_decay, (int, float)) and not isinstance(layer_decay, bool) and 0.0 < layer_decay <= 1.0):
        raise ValueError(f"layer_decay must be in (0, 1] or None, got {layer_decay!r}")
    for key, m in mults.items():
        if isinstance(m, bool) or not isinstance(m, (int, float)) or not (m > 0.0) or math.isinf(m):
            raise ValueError(f"{key} must be a positive number, got {m!r}")


def build_param_groups(model, lr, weight_decay, layer_decay=None, no_decay_1d=False, image_lr_mult=1.0, text_lr_mult=1.0):
    """-> [{'params', 'lr', 'weight_decay', 'name'}]: every parameter of `model` in exactly one group (frozen ones too, as the reference
    lists them: the checkpoint layout depends on it), groups in the order of their first parameter in `model.parameters()`."""
    _check(layer_decay, {"image_lr_mult": image_lr_mult, "text_lr_mult": text_lr_mult})
    named = list(model.named_parameters())
    if layer_decay is None and not no_decay_1d and image_lr_mult == 1.0 and text_lr_mult == 1.0:
        return [dict(params=[p for _, p in named], lr=lr, weight_decay=weight_decay, name="all")]
    towers = []                                            # (prefix of the full names, kind, {relative name: id}, L)
    for mod_name, mod in model.named_modules():
        prefix = (mod_name + "." if mod_name else "") + "model."
        if _is_tower(mod) and not any(prefix.startswith(t[0]) for t in towers):
            rel = [n for n, _ in mod.model.named_parameters()]
            towers.append((prefix, tower_kind(rel)) + layer_ids(rel))
    groups = {}
    for name, p in named:
        tag, scale, layer = "head", 1.0, None
        for prefix, kind, ids, L in towers:
            if name.startswith(prefix):
                tag = "text" if kind == "bert" else "image"
                scale = float(text_lr_mult if kind == "bert" else image_lr_mult)
                if layer_decay is not None and layer_decay != 1.0 and ids:
                    layer = ids[name[len(prefix):]]
                    scale *= float(layer_decay) ** (L - layer)
                break
        plain = bool(no_decay_1d) and is_no_decay(name, p)
        key = (tag, layer, plain)
        if key not in groups:
            label = tag + ("" if layer is None else f".layer{layer:02d}") + (".no_decay" if plain else "")
            groups[key] = dict(params=[], lr=lr * scale, weight_decay=0.0 if plain else weight_decay, name=label)
        groups[key]["params"].append(p)
    return list(groups.values())


def group_table(groups):
    """One line per group for the log: name, tensor count, element count, lr, weight decay."""
    width = max(len(str(g.get("name", i))) for i, g in enumerate(groups))
    rows = [f"| {'group'.ljust(width)} | tensors |    elements |        lr | weight_decay |"]
    for i, g in enumerate(groups):
        rows.append(f"| {str(g.get('name', i)).ljust(width)} | {len(g['params']):>7} | {sum(p.numel() for p in g['params']):>11} | "
                    f"{g['lr']:.3e} | {g['weight_decay']:>12.3e} |")
    return "\n".join(rows)
