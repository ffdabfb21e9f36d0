"""Fused AdamW over the towers' flat parameter arenas (csrc/norm_elementwise.hip: mmg_adamw_step) with
torch.optim.AdamW semantics (mmgclip/experiments/ClassifierExperiment.py:74: lr 5e-5, weight_decay 1e-4, default betas).

Arena-backed parameters (ConvNeXt / ViT / ResNet / BERT towers) are updated by ONE launch per tower; any other parameter
(projection heads, logit_scale) gets one launch per tensor.  The arenas are found from the parameters themselves
(`ParamArena` leaves a back-pointer on each parameter it binds), at every `step()`: the towers build their arenas at their
first forward, which is AFTER the reference's construction order builds the optimizer (ClassifierExperiment.py:65-74).
The one-launch path is taken when every parameter of an arena is trainable, in this optimizer, and has its gradient in the
arena's flat gradient buffer; otherwise its trainable parameters are updated one by one and the arena is told so
(`touch()`), which is what makes the towers rebuild their bf16 working copies.

Param groups (no-decay sets, layer-wise learning rates: optim_groups.build_param_groups): an arena is considered once per step, across
all groups.  Sitting in one group it takes the launch above, symbol for symbol; spread over several groups that share `betas` and `eps`
it still goes out as ONE launch (csrc/adamw_groups.hip: mmg_adamw_step_groups), with a cached one-byte-per-64-elements map from chunk
to group on the device and the groups' `lr` / `weight_decay` read from `param_groups` at every step and passed by value.  Mixed
`betas` / `eps`, more than 128 distinct (lr, weight_decay) pairs, a partly frozen arena and loose tensors take the per-tensor path,
each tensor with its own group's values.

State layout = torch.optim.AdamW's: `state[p] = {'step': fp32 0-d tensor, 'exp_avg', 'exp_avg_sq'}`, so
`state_dict()` / `load_state_dict()` (what EarlyStopper writes as 'optimizer_state_dict', callbacks/early_stopping.py:52-65)
round-trip and are interchangeable with the reference's torch.optim.AdamW PROVIDED both list the same parameters in the same order:
the reference passes `model.parameters()` - frozen BERT included - and so does ClassifierExperiment here (parameters without a
gradient are skipped and get no state, as in torch).  For arena parameters `exp_avg` / `exp_avg_sq` are
views into two flat buffers (rebuilt from the per-parameter tensors after a load).

`max_grad_norm` / `skip_nonfinite` (additive; off by default, and then `step()` issues exactly the launches it always did): clip the
gradients by their global L2 norm, as torch.nn.utils.clip_grad_norm_ over every gradient this optimizer applies, and leave
parameters and moments untouched when that norm is NaN or Inf (csrc/grad_clip.hip).  `skip_nonfinite` defaults to True when
`max_grad_norm` is given and to off when it is not; `skip_nonfinite=True` alone guards without clipping.  With
`max_grad_norm` set and `skip_nonfinite=False` nothing is held back: a NaN norm gives a NaN coefficient, which the AdamW launches
write into every parameter and moment - exactly what clip_grad_norm_ (error_if_nonfinite=False) followed by torch.optim.AdamW does.
One exception to "reads nothing back": a state created AFTER guarded steps have run (a parameter unfrozen mid-run) reads the
skipped count once, at that step, to start its counter there (`_new_counter`).  The norm, the coefficient, the decision and
the count of skipped steps stay on the device: `step()` reads nothing back.  The host step counters keep counting `step()` calls;
Adam's clock is `step - skipped` on the device, and `state_dict()` writes that difference, which is what torch.optim.AdamW would
have written had the bad steps not been taken."""
import math

import torch

from . import kernels as K


def build_chunk_map(arena, slots):
    """uint8 [arena.size / 64] on the host: the slot (`slots[i]` of the i-th arena parameter) of every 64-element chunk.  ParamArena starts
    each parameter on a 64-element boundary, so a chunk belongs to exactly one parameter; the padding behind a parameter is part of its
    last chunk (zero in the gradient and the moments, so it stays zero whatever the slot's hyper-parameters are)."""
    assert arena.size % 64 == 0 and len(slots) == len(arena.params)
    out = torch.empty(arena.size // 64, dtype=torch.uint8)
    for n, p, s in zip(arena.names, arena.params, slots):
        assert 0 <= s < 256 and arena.offsets[n] % 64 == 0
        first = arena.offsets[n] // 64
        out[first:first + (p.numel() + 63) // 64] = s
    return out


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, arenas=(), max_grad_norm=None,
                 skip_nonfinite=None):
        if max_grad_norm is not None and not (float(max_grad_norm) > 0.0):
            raise ValueError(f"max_grad_norm must be a positive number or None, got {max_grad_norm!r}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        # `arenas` is accepted for backward compatibility; arenas are discovered from the parameters at step time
        self._flat = {}              # id(arena) -> dict(arena, m, v, step)
        self.max_grad_norm = None if max_grad_norm is None or math.isinf(float(max_grad_norm)) else float(max_grad_norm)
        # skip_nonfinite=None: True beside a max_grad_norm, off without one - so that FusedAdamW(params, lr=...) stays the unguarded
        # step, launch for launch, while skip_nonfinite=True on its own guards without clipping
        self.skip_nonfinite = (max_grad_norm is not None) if skip_nonfinite is None else bool(skip_nonfinite)
        self.grad_norm = None        # device fp32 [4] of the last guarded step: total norm, clip coefficient, 1 = finite, spare
        self._skipped = None         # device int32 [1]: guarded steps that were not applied since the counters were last loaded
        self._clock_running = False  # a guarded step has run since then (a state created later starts at the skipped count)
        self._partials, self._piece_sizes, self._piece_counts = None, None, None

    # ---- state plumbing --------------------------------------------------------------------------------------------
    def _flat_state(self, arena):
        """Flat moment buffers of an arena, with every parameter's `exp_avg` / `exp_avg_sq` a view into them."""
        fs = self._flat.get(id(arena))
        p0 = arena.params[0]
        bound = fs is not None and fs["arena"] is arena and "exp_avg" in self.state[p0] and \
            self.state[p0]["exp_avg"].data_ptr() == fs["m"].data_ptr() + 4 * arena.offsets[arena.names[0]]
        if bound:
            return fs
        m, v = torch.zeros_like(arena.data), torch.zeros_like(arena.data)
        step = self._new_counter()
        for n, p in zip(arena.names, arena.params):
            o = arena.offsets[n]
            mv, vv = m[o:o + p.numel()].view(p.shape), v[o:o + p.numel()].view(p.shape)
            st = self.state[p]
            if "exp_avg" in st:                                  # loaded from a checkpoint (or updated per tensor so far)
                mv.copy_(st["exp_avg"])
                vv.copy_(st["exp_avg_sq"])
                step = torch.maximum(step, torch.as_tensor(st["step"], dtype=torch.float32).cpu().reshape(()))
            st["exp_avg"], st["exp_avg_sq"] = mv, vv
        for p in arena.params:
            self.state[p]["step"] = step                         # one shared counter: the arena is stepped as a whole
        fs = self._flat[id(arena)] = dict(arena=arena, m=m, v=v, step=step)
        return fs

    def state_dict(self):
        """torch.optim.AdamW's layout.  The parameters of an arena share ONE live step counter; a serialised state gets a counter
        of its own per parameter, as torch writes it (torch's foreach step increments every counter it is handed: a tensor listed
        178 times would be incremented 178 times per step).  With the non-finite guard on, the counters are written minus the steps
        that were skipped (one read-back): the checkpoint torch.optim.AdamW would have written, not having taken those steps."""
        sd = super().state_dict()
        k = self.skipped_steps()
        sd["state"] = {i: {kk: ((vv - k).clamp_(min=0) if k else vv.clone()) if kk == "step" and torch.is_tensor(vv) else vv
                           for kk, vv in v.items()} for i, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """The loaded counters are Adam's clock itself: the device count of skipped steps starts again at zero."""
        super().load_state_dict(state_dict)
        if self._skipped is not None:
            self._skipped.zero_()
        self._clock_running = False

    def skipped_steps(self):
        """Guarded steps whose gradient norm was not finite and that were therefore not applied (one read-back, on request)."""
        return int(self._skipped.item()) if self._skipped is not None else 0

    def _new_counter(self):
        """Step counter of a state created now.  Adam's clock is `step - skipped` with ONE device count of skipped steps, so a state that
        joins after guarded steps have run (a parameter unfrozen mid-run) starts at that count - the only read-back `step()` can make,
        and only at such a join."""
        return torch.full((), float(self.skipped_steps() if self._clock_running else 0), dtype=torch.float32)

    def _tensor_state(self, p):
        st = self.state[p]
        if "exp_avg" not in st:
            st["step"] = self._new_counter()
            st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p.data), torch.zeros_like(p.data)
        elif not st["exp_avg"].is_contiguous() or st["exp_avg"].device != p.device:
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].to(p.device).contiguous(), st["exp_avg_sq"].to(p.device).contiguous()
        if not torch.is_tensor(st["step"]):
            st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
        return st

    # ---- the step --------------------------------------------------------------------------------------------------
    def _grouped_launch(self, arena, group_of):
        """A whole arena whose parameters sit in several param groups -> (device chunk map, [lr per slot], [weight_decay per slot]) for
        ONE mmg_adamw_step_groups launch, or None when the launch cannot express it (the groups differ in betas / eps, or span more
        than 128 distinct (lr, weight_decay) pairs).  A slot is a param group; only beyond 128 groups are groups of equal (lr,
        weight_decay) merged.  lr / weight_decay are read here, at every step; the map is cached on the arena's flat state and rebuilt
        when the arena was rebuilt (new flat state) or a parameter's slot changed."""
        owners = [group_of[id(p)] for p in arena.params]
        used = sorted(set(owners))
        groups = [self.param_groups[gi] for gi in used]
        if any(tuple(g["betas"]) != tuple(groups[0]["betas"]) or g["eps"] != groups[0]["eps"] for g in groups[1:]):
            return None
        pairs = [(float(g["lr"]), float(g["weight_decay"])) for g in groups]
        if len(used) <= K.ADAMW_MAX_GROUPS:
            slot_of = {gi: s for s, gi in enumerate(used)}
        else:
            distinct = list(dict.fromkeys(pairs))
            if len(distinct) > K.ADAMW_MAX_GROUPS:
                return None
            slot_of = {gi: distinct.index(pair) for gi, pair in zip(used, pairs)}
            pairs = distinct
        slots = tuple(slot_of[gi] for gi in owners)
        fs = self._flat_state(arena)
        if fs.get("slots") != slots:
            fs["slots"], fs["chunk_map"] = slots, build_chunk_map(arena, slots).to(arena.data.device)
        return fs["chunk_map"], [lr for lr, _ in pairs], [wd for _, wd in pairs]

    def _collect(self):
        """Every update this step will make, each gradient exactly once: [(p, g, m, v, (lr, b1, b2, eps, wd), step, grouped)] - a whole
        arena as ONE flat entry (its 64-element padding gaps are zero in the gradient and stay zero; `grouped` = `_grouped_launch`'s
        result when it sits in several groups, whose lr / wd then replace the entry's own), anything else per tensor - and the
        arenas that must be told their parameters moved.  Advances the host step counters; launches nothing but state set-up."""
        jobs, touched, done = [], {}, set()
        group_of = {id(p): gi for gi, group in enumerate(self.param_groups) for p in group["params"]}
        for group in self.param_groups:
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            hyper = (lr, b1, b2, eps, wd)
            arenas = {}
            for p in group["params"]:
                a = getattr(p, "_mmg_arena", None)
                if a is not None and a.is_bound() and id(p) not in done:
                    arenas[id(a)] = a
            for arena in arenas.values():        # an arena is considered once per step, at the first group that lists one of its parameters
                whole = all(p.requires_grad and id(p) in group_of and p.grad is not None and
                            p.grad.data_ptr() == arena.g(n).data_ptr() for n, p in zip(arena.names, arena.params))
                if not whole:
                    continue
                grouped = None
                if len({group_of[id(p)] for p in arena.params}) > 1:
                    grouped = self._grouped_launch(arena, group_of)
                    if grouped is None:          # mixed betas / eps, or too many groups: per tensor, each with its own group's values
                        continue
                fs = self._flat_state(arena)
                fs["step"] += 1
                jobs.append((arena.data, arena.grad, fs["m"], fs["v"], hyper, int(fs["step"]), grouped))
                touched[id(arena)] = arena
                done.update(id(p) for p in arena.params)
            for p in group["params"]:
                if p.grad is None or id(p) in done:
                    continue
                if not p.data.is_contiguous():
                    raise RuntimeError("FusedAdamW needs contiguous parameters")
                st = self._tensor_state(p)
                if st["step"].data_ptr() in {fs["step"].data_ptr() for fs in self._flat.values()}:
                    st["step"] = st["step"].clone()              # leaving the whole-arena path: own counter from here on
                st["step"] += 1
                jobs.append((p.data, p.grad.contiguous(), st["exp_avg"], st["exp_avg_sq"], hyper, int(st["step"]), None))
                a = getattr(p, "_mmg_arena", None)
                if a is not None:                # the update goes through a raw pointer: p._version does not move, say so
                    touched[id(a)] = a
        return jobs, list(touched.values())

    def _clip_state(self, grads):
        """Global norm of `grads` -> self.grad_norm (device), skipped-step count (device): one streaming reduction per gradient into
        one fp64 partials buffer, one finalize launch.  The buffers are cached and re-made when the gradients' sizes change."""
        dev = grads[0].device
        sizes = tuple(g.numel() for g in grads)
        if self._piece_sizes != sizes or self._partials.device != dev:
            self._piece_counts = [K.grad_sumsq_partials(n) for n in sizes]
            self._partials = torch.empty(sum(self._piece_counts), device=dev, dtype=torch.float64)
            self._piece_sizes = sizes
        if self.grad_norm is None or self.grad_norm.device != dev:
            self.grad_norm = torch.zeros(4, device=dev, dtype=torch.float32)
            self._skipped = torch.zeros(1, device=dev, dtype=torch.int32) if self.skip_nonfinite else None
        off = 0
        for g, c in zip(grads, self._piece_counts):
            K.grad_sumsq(g, self._partials, off, c)
            off += c
        K.grad_clip_finalize(self._partials, off, self.max_grad_norm, self.grad_norm, self._skipped)
        self._clock_running = True
        return self.grad_norm, self._skipped

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        guarded = self.max_grad_norm is not None or self.skip_nonfinite
        jobs, touched = self._collect()
        if guarded and jobs:
            # no .item(), no .cpu(), no synchronisation: the coefficient, the go/no-go and Adam's clock are read by the AdamW launches
            clip, skipped = self._clip_state([j[1] for j in jobs])
        else:
            clip = skipped = None
        for p, g, m, v, hyper, t, grouped in jobs:
            if grouped is not None:              # a whole arena in several groups: one launch, lr / weight_decay per 64-element chunk
                chunk_map, lrs, wds = grouped
                K.adamw_step_groups(p, g, m, v, chunk_map, lrs, wds, hyper[1], hyper[2], hyper[3], t, clip, skipped)
            elif clip is not None:
                K.adamw_step_guarded(p, g, m, v, None, *hyper, t, clip, skipped)
            else:
                K.adamw_step(p, g, m, v, None, *hyper, t)
        for a in touched:        # (on a skipped step too: harmless, the towers re-cast unchanged parameters)
            a.touch()
        return loss
