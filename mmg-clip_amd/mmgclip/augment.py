"""Seeded augmentation of the pixel towers' input - decided here, on the host, as plain values (no tensors, no device), in the style of
networks/convnext_sd.py.  The pixels are touched once, by `mmg_patchify_aug` (csrc/pixel_input.hip), which applies per image, in this order,
    flip (over the full H, W) -> integer shift (ty, tx) -> fill (raw 0, black) -> tone (gain * x + offset, clamped to [0, 1]) -> 16-bit scaling
from two small tables: geom int32 [n, 4] = (flags: bit0 flip x, bit1 flip y; ty; tx; 0) and tone fp32 [n, 2] = (gain, offset).

  * `AugmentSpec`   hflip, vflip: probabilities in [0, 1]; max_shift: pixels, >= 0; gain: [lo, hi] with 0 < lo <= hi; offset: [lo, hi].
  * `draw`          (spec, seed, sample_ids) -> (geom rows, tone rows).  The counter-based hash of csrc/dropout.h (fmix32, mmg_drop_key,
                    mmg_drop_bits - networks/convnext_sd.py restates it in numpy, and this module uses that restatement): every quantity draws
                    under a site of its own, indexed by the image's position in the forward's INPUT, so a row is a pure function of
                    (seed, sample id) - it does not depend on the micro-batch size, on the grouping of a list of images by size, or on
                    whether a pass is a checkpointed recomputation.
  * `AugmentSeeds`  one seed per recorded forward, a DropSeeds stream with an additive constant of its own (unrelated to the
                    stochastic-depth stream and to the text tower's dropout), restarted from (base seed, rank) by `seeding(s)`.

The mapping, exactly.  bits_q(i) = mmg_drop_bits(sample_ids[i], mmg_drop_key(seed, SITE_q)), a 32-bit number, for the six sites
SITE_HFLIP, SITE_VFLIP, SITE_TY, SITE_TX, SITE_GAIN, SITE_OFFSET = 0x100 .. 0x105 (the shift's two components draw apart):
    flip x   iff  bits_hflip < mmg_drop_threshold(hflip) = floor(hflip * 2^32) (capped at 2^32 - 1), or hflip == 1     (flags bit 0)
    flip y   iff  the same with vflip under its own site                                                                  (flags bit 1)
    ty       =    bits_ty % (2 * max_shift + 1) - max_shift      (tx likewise under its site; the modulo's bias is < 2^-20 per value at 2048)
    gain     =    lo + (hi - lo) * u,  u = (bits_gain >> 8) / 2^24 in [0, 1), evaluated in double; the table holds its fp32 rounding
    offset   =    the same under its site
so hflip = vflip = 0, max_shift = 0, gain = [1, 1], offset = [0, 0] draws identity rows ((0, 0, 0, 0) and (1.0, 0.0)) for every id."""
from typing import NamedTuple, Tuple

import numpy as np

from .networks.convnext_sd import _M32, DropSeeds, _fmix32, drop_key, drop_threshold

SITE_HFLIP, SITE_VFLIP, SITE_TY, SITE_TX, SITE_GAIN, SITE_OFFSET = 0x100, 0x101, 0x102, 0x103, 0x104, 0x105
_KEYS = ("hflip", "vflip", "max_shift", "gain", "offset")


class AugmentSpec(NamedTuple):
    hflip: float = 0.0
    vflip: float = 0.0
    max_shift: int = 0
    gain: Tuple[float, float] = (1.0, 1.0)
    offset: Tuple[float, float] = (0.0, 0.0)


def _number(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError(f"augment.{what} must be a finite number, got {v!r}")
    return v


def _pair(v, what):
    try:
        lo, hi = (float(_number(x, what)) for x in v)
    except TypeError:
        raise ValueError(f"augment.{what} must be [lo, hi], got {v!r}") from None
    except ValueError as e:
        raise ValueError(f"augment.{what} must be [lo, hi] of two finite numbers, got {v!r}") from e
    if lo > hi:
        raise ValueError(f"augment.{what} must be [lo, hi] with lo <= hi, got {v!r}")
    return lo, hi


def make_spec(spec):
    """None | AugmentSpec | mapping (a config node: anything with keys() and item access) -> a validated AugmentSpec, or None.
    Unknown keys, probabilities outside [0, 1], a negative or fractional max_shift, gain with lo <= 0 or lo > hi raise ValueError."""
    if spec is None:
        return None
    if isinstance(spec, AugmentSpec):
        vals = spec._asdict()
    elif hasattr(spec, "keys"):
        vals = {k: spec[k] for k in spec.keys()}
    else:
        raise ValueError(f"augment must be None, an AugmentSpec or a mapping, got {type(spec).__name__}")
    unknown = sorted(set(vals) - set(_KEYS))
    if unknown:
        raise ValueError(f"augment: unknown key(s) {unknown}; known: {list(_KEYS)}")
    out = AugmentSpec()._asdict()
    for k in ("hflip", "vflip"):
        if k in vals:
            p = float(_number(vals[k], k))
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"augment.{k} is a probability in [0, 1], got {p}")
            out[k] = p
    if "max_shift" in vals:
        m = _number(vals["max_shift"], "max_shift")
        if m < 0 or m != int(m) or m > 2 ** 30:
            raise ValueError(f"augment.max_shift must be a whole number of pixels >= 0, got {m!r}")
        out["max_shift"] = int(m)
    if "gain" in vals:
        out["gain"] = _pair(vals["gain"], "gain")
        if out["gain"][0] <= 0.0:
            raise ValueError(f"augment.gain must be [lo, hi] with 0 < lo <= hi, got {vals['gain']!r}")
    if "offset" in vals:
        out["offset"] = _pair(vals["offset"], "offset")
    return AugmentSpec(**out)


def _bits(seed, site, ids):
    """mmg_drop_bits(ids, mmg_drop_key(seed, site)) as uint64 holding 32-bit values."""
    return _fmix32((ids * np.uint64(0x9E3779B1) + np.uint64(drop_key(seed, site))) & _M32)


def draw(spec, seed, sample_ids):
    """-> (geom rows: [flags, ty, tx, 0] ints, tone rows: [gain, offset] floats), one per entry of sample_ids (module docstring)."""
    spec = make_spec(spec)
    ids = np.asarray(list(sample_ids), dtype=np.uint64).reshape(-1) & _M32

    def flips(p, site):
        return np.ones(ids.size, dtype=bool) if p >= 1.0 else _bits(seed, site, ids) < np.uint64(drop_threshold(p))

    def shifts(site):
        m = spec.max_shift
        return (_bits(seed, site, ids) % np.uint64(2 * m + 1)).astype(np.int64) - m

    def uniform(lohi, site):
        lo, hi = lohi
        return lo + (hi - lo) * ((_bits(seed, site, ids) >> np.uint64(8)).astype(np.float64) / 16777216.0)

    flags = flips(spec.hflip, SITE_HFLIP).astype(np.int64) | (flips(spec.vflip, SITE_VFLIP).astype(np.int64) << 1)
    ty, tx = shifts(SITE_TY), shifts(SITE_TX)
    gain, offset = uniform(spec.gain, SITE_GAIN), uniform(spec.offset, SITE_OFFSET)
    geom = [[int(f), int(y), int(x), 0] for f, y, x in zip(flags, ty, tx)]
    tone = [[float(g), float(o)] for g, o in zip(gain, offset)]
    return geom, tone


class AugmentSeeds(DropSeeds):
    """The augmentation's private seed stream: DropSeeds' derivation from (base seed, rank) under another additive constant."""
    ADD = 0x94D049BB133111EB
