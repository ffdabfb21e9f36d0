"""What the four towers share (mmgclip.networks.tower), without a GPU and without the kernel library: the micro-batch / checkpointing
schedule driven with fakes that log their calls, the Tower base class on a toy CPU model, and the convolution-weight layout against the three
expressions it replaced."""
import gc
import weakref

import pytest
import torch
import torch.nn as nn

from mmgclip.networks.tower import Recompute, Tower, backward_parts, checkpoint_plan, conv_weight_rows, forward_parts

CPU = torch.device("cpu")


# ---- the schedule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, ckpt, keep_last, recompute, order", [
    (1, True, True, [False], [0]),
    (3, True, True, [True, True, False], [2, 1, 0]),
    (3, True, False, [True, True, True], [2, 1, 0]),
    (3, False, True, [False, False, False], [0, 1, 2]),
    (3, False, False, [False, False, False], [0, 1, 2]),
])
def test_checkpoint_plan(n, ckpt, keep_last, recompute, order):
    assert checkpoint_plan(n, ckpt, keep_last) == (recompute, order)


class _State:
    """Stands for a micro-batch's saved activations (an object a weak reference can watch)."""

    def __init__(self, part):
        self.part = part


# mode -> (ckpt, MMG_CKPT_KEEP_LAST, parts recomputed)
MODES = {"plain": (False, "1", []), "keep_last": (True, "1", [0, 1]), "recompute_all": (True, "0", [0, 1, 2])}


@pytest.mark.parametrize("mode", list(MODES))
def test_drivers_schedule_slices_and_release(mode, monkeypatch):
    ckpt, keep_last, recomputed = MODES[mode]
    monkeypatch.setenv("MMG_CKPT_KEEP_LAST", keep_last)
    pixels = torch.arange(5 * 3, dtype=torch.float32).reshape(5, 3)            # parts of 2, 2 and 1 rows; row i starts with 3 i
    bounds = [(0, 2), (2, 4), (4, 5)]
    log, states = [], []
    part_of = lambda x: int(x[0, 0].item()) // 6                              # noqa: E731  (first rows 0, 2, 4 -> parts 0, 1, 2)

    def make_part(a, b):
        def part():
            log.append(("input", a // 2))
            return pixels[a:b]
        return part

    def state(k):
        s = _State(k)
        states.append(weakref.ref(s))
        return s

    def run(x, saving):
        log.append(("run", part_of(x), saving))
        return 2 * x, (state(part_of(x)) if saving else None)

    feat, rec = forward_parts([make_part(a, b) for a, b in bounds], run, ckpt)
    assert torch.equal(feat, 2 * pixels)
    # the forward: every part once, in order; a part that will be recomputed runs with saving=False and leaves only a Recompute record
    assert log == [e for k in range(3) for e in (("input", k), ("run", k, k not in recomputed))]
    assert rec.rows == [2, 2, 1]
    for k in range(3):
        if k in recomputed:
            assert isinstance(rec.records[k], Recompute) and rec.records[k].rows == rec.rows[k]
        else:
            assert isinstance(rec.records[k], _State) and rec.records[k].part == k
    assert len(states) == 3 - len(recomputed)

    del log[:]
    dfeat = torch.arange(5 * 3, dtype=torch.float32).reshape(5, 3) + 100.0

    def recompute_run(x):
        log.append(("recompute", part_of(x)))
        return state(part_of(x))

    def bwd(d, saved, last):
        assert isinstance(saved, _State)
        log.append(("bwd", saved.part, d.clone(), last))

    backward_parts(rec, dfeat, recompute_run, bwd)
    order = [2, 1, 0] if ckpt else [0, 1, 2]
    want = []
    for k in order:
        if k in recomputed:                     # the pixels are built again and the forward re-run directly before this part's backward
            want += [("input", k), ("recompute", k)]
        want.append(("bwd", k))
    assert [e[:2] for e in log] == want
    calls = [e for e in log if e[0] == "bwd"]
    for _, k, d, _ in calls:                    # exactly the part's rows of the feature gradient
        assert torch.equal(d, dfeat[bounds[k][0]:bounds[k][1]]), k
    assert [last for *_, last in calls] == [False, False, True]
    # nothing saved is referenced any more: neither by the record nor by the drivers
    assert rec.records == [None, None, None]
    del calls, log
    gc.collect()
    assert len(states) == 3 and all(s() is None for s in states)


def test_keep_last_is_read_once_per_forward(monkeypatch):
    """The knob belongs to the forward: a backward under another value follows what its forward recorded."""
    monkeypatch.setenv("MMG_CKPT_KEEP_LAST", "0")
    x = torch.ones(4, 1)
    _, rec = forward_parts([lambda: x[:2], lambda: x[2:]], lambda t, saving: (t, "saved" if saving else None), True)
    monkeypatch.setenv("MMG_CKPT_KEEP_LAST", "1")
    seen = []
    backward_parts(rec, x, lambda t: seen.append("recompute") or "again", lambda d, saved, last: seen.append(saved))
    assert seen == ["recompute", "again", "recompute", "again"]


# ---- the base class -----------------------------------------------------------------------------------------------------------------------
class _Toy(Tower):
    def __init__(self):
        super().__init__()
        self.model = nn.Sequential(nn.Linear(4, 3), nn.ReLU(), nn.Linear(3, 2))
        self.builds = self.bounds = 0
        self.key = None

    def _bound(self):
        self.bounds += 1

    def _working_copy_key(self):
        return super()._working_copy_key() if self.key is None else self.key

    def _build_working_copies(self):
        self.builds += 1
        return {"n": self.builds}


def test_tower_starts_unbound():
    t = _Toy()
    assert t._arena is None and t.arena is None and t._wc is None and t._wc_version is None and t.post_backward_hook is None


def test_materialize_binds_once_and_rebuilds_when_a_parameter_was_replaced():
    t = _Toy()
    want = {n: p.detach().clone() for n, p in t.model.named_parameters()}
    t._materialize(CPU)
    arena = t.arena
    assert arena is t._arena and arena.is_bound() and t.bounds == 1
    assert arena.names == list(want)                                         # the default: every parameter of `model`, in its order
    for n, p in t.model.named_parameters():
        assert p._mmg_arena is arena and torch.equal(p.data, want[n])
    t._materialize(CPU)
    assert t.arena is arena and t.bounds == 1
    p0 = t.model[0].weight
    p0.data = p0.data.clone()                                                # (what .to(device) or a loaded checkpoint may do)
    assert not arena.is_bound()
    t._refresh_working_copies()
    assert t._wc_version is not None
    t._materialize(CPU)
    assert t.arena is not arena and t.arena.is_bound() and t.bounds == 2 and p0._mmg_arena is t.arena
    assert t._wc_version is None                                             # the working copies of the old arena are not current


def test_working_copies_are_rebuilt_only_when_a_parameter_changed():
    t = _Toy()
    t._materialize(CPU)
    t._refresh_working_copies()
    assert t.builds == 1 and t._wc == {"n": 1}
    t._refresh_working_copies()
    assert t.builds == 1
    with torch.no_grad():
        t.model[2].bias.add_(1.0)                                            # in place: the parameter's version moves
    t._refresh_working_copies()
    assert t.builds == 2 and t._wc == {"n": 2}
    t.arena.touch()                                                          # (a fused optimizer writes the flat buffer directly)
    t._refresh_working_copies()
    t._refresh_working_copies()
    assert t.builds == 3
    t.key = "a"                                                              # an overridden key decides alone
    t._refresh_working_copies()
    t.arena.touch()
    t._refresh_working_copies()
    assert t.builds == 4 and t._wc_version == "a"
    t.key = "b"
    t._refresh_working_copies()
    assert t.builds == 5


def test_record_forward_counts_only_forwards_that_get_a_backward():
    t = _Toy()
    with torch.no_grad():
        assert t._record_forward(CPU) is None
    assert t.arena.is_bound() and t.arena.open_backwards == 0                # (it binds the parameters either way)
    assert t._record_forward(CPU, wants_grad=False) is None and t.arena.open_backwards == 0
    for p in t.model.parameters():
        p.requires_grad = False
    assert t._record_forward(CPU) is None and t.arena.open_backwards == 0
    t.model[0].weight.requires_grad = True
    a = t._record_forward(CPU)
    assert a.is_leaf and a.requires_grad and a.device == CPU and t.arena.open_backwards == 1
    assert t._record_forward(CPU) is a and t.arena.open_backwards == 2       # (one anchor per stream; one count per recorded forward)


def test_towers_choose_what_goes_into_the_arena():
    from mmgclip.networks.bert import BertConfigLite, BertTower
    from mmgclip.networks.resnet import ResNetTower
    bert = BertTower(BertConfigLite(vocab_size=50, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128,
                                    max_position_embeddings=16))
    bert._materialize(CPU)                                                   # (BERT checks the Q/K/V spans of the arena it was given)
    names = bert.arena.names
    assert sorted(names) == sorted(n for n, _ in bert.model.named_parameters())
    i = names.index("encoder.layer.1.attention.self.query.weight")
    assert names[i:i + 6] == [f"encoder.layer.1.attention.self.{x}.{leaf}" for leaf in ("weight", "bias") for x in ("query", "key", "value")]
    resnet = ResNetTower()
    resnet._materialize(CPU)
    assert resnet.arena.names == ["layer4." + n for n, _ in resnet.model.layer4.named_parameters()]
    key = resnet._working_copy_key()
    with torch.no_grad():
        resnet.model.conv1.weight.mul_(0.5)                                  # a frozen parameter, outside the arena, still has a working copy
    assert resnet._working_copy_key() != key and resnet.arena.version() == key[0]


# ---- convolution weights as GEMM rows -------------------------------------------------------------------------------------------------
def _weight(co, ci, kh, kw):
    return torch.randn(co, ci, kh, kw, generator=torch.Generator().manual_seed(co + kh))


def _patch_conv_rows(w, kp):
    """The ConvNeXt stem's and the ViT patch projection's former spelling."""
    rows = torch.zeros(w.shape[0], kp)
    rows[:, :w.shape[2] * w.shape[3] * w.shape[1]] = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    return rows


def _resnet_rows(w, cin_pad=None):
    """ResNetTower._w2d's former body."""
    co, ci, kh, kw = w.shape
    if cin_pad and cin_pad > ci:
        w = torch.cat([w, torch.zeros(co, cin_pad - ci, kh, kw)], 1)
        ci = cin_pad
    w = w.permute(0, 2, 3, 1).reshape(co, kh * kw * ci)
    kp = (w.shape[1] + 31) // 32 * 32
    if kp != w.shape[1]:
        w = torch.cat([w, torch.zeros(co, kp - w.shape[1])], 1)
    return w.contiguous()


@pytest.mark.parametrize("shape, cin_pad, width, old", [
    ((96, 1, 4, 4), None, 32, lambda w: _patch_conv_rows(w, 32)),                                    # ConvNeXt stem
    ((64, 1, 16, 16), None, 256, lambda w: _patch_conv_rows(w, 256)),                                # ViT conv_proj
    ((64, 3, 7, 7), 8, 416, lambda w: _resnet_rows(w, 8)),                                           # ResNet conv1: 7 * 7 * 8 = 392 -> 416
    ((64, 32, 3, 3), None, 288, _resnet_rows),                                                       # ResNet conv2
    ((192, 96, 2, 2), None, 384, lambda w: w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()),   # ConvNeXt downsample: no padding
])
def test_conv_weight_rows_equals_the_expressions_it_replaced(shape, cin_pad, width, old):
    w = _weight(*shape)
    rows = conv_weight_rows(w, cin_pad)
    assert rows.shape == (shape[0], width) and rows.dtype == torch.float32 and rows.is_contiguous()
    assert torch.equal(rows, old(w))
