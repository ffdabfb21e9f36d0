"""Patch dropout of the ViT tower (FLIP, Li et al. 2023; open_clip's `patch_dropout`) - decided here, on the host, as plain values, in the
style of networks/convnext_sd.py and augment.py.  Under train() every image keeps K of its P patches plus the class token; the encoder runs
on 1 + K tokens; eval() sees every patch.  The device makes the same draw in `mmg_patch_keep_indices` (csrc/patch_dropout.hip); this module
is the statement of record and what the tests compare that kernel against.

  * `check_rate`     rate in [0, 1), else ValueError.
  * `keep_count`     K = max(1, int(P * (1.0 - rate))): open_clip's rule, in Python doubles.  Every image keeps the same K (rectangular shapes).
  * `keep_indices`   (seed, sample_ids, P, K) -> (keep int32 [B, K], slot int32 [B, P]).
  * `PatchDropSeeds` one seed per forward that drops, a DropSeeds stream with an additive constant of its own (unrelated to the augmentation's,
                     to stochastic depth's and to the text tower's dropout), restarted from (base seed, rank) by `seeding(s)`.

The mapping, exactly (csrc/dropout.h; networks/convnext_sd.py restates fmix32 and mmg_drop_key in numpy and this module uses them):
    key0   = mmg_drop_key(seed, SITE)                        SITE = 0x50447270
    key_i  = mmg_drop_key_bh(key0, (uint32) sample_id)       = fmix32(key0 + sample_id * 0xB5297A4D)
    bits_p = mmg_drop_bits(p, key_i)                         = fmix32(p * 0x9E3779B1 + key_i),   p = 0 .. P-1
Image i keeps the K patches with the smallest bits_p, in ascending patch order.  mmg_drop_bits is a bijection of the 32-bit p (an odd
multiplier, an added constant, the invertible murmur3 finaliser), so two patches of one image never draw equal bits: no tie rule is needed.
A row is a pure function of (seed, sample id): it does not depend on the micro-batch size or on whether a pass is a checkpointed
recomputation.  slot[i, p] is the position of patch p among the kept patches of image i, or -1."""
import numpy as np

from .networks.convnext_sd import _M32, DropSeeds, _fmix32, drop_key

SITE = 0x50447270
MAX_PATCHES = 16384                     # what the kernel's LDS layout holds (one workgroup per image)


def check_rate(rate):
    if isinstance(rate, bool) or not isinstance(rate, (int, float, np.integer, np.floating)):
        raise ValueError(f"patch_dropout must be a number in [0, 1), got {rate!r}")
    rate = float(rate)
    if not 0.0 <= rate < 1.0:           # (NaN fails both comparisons)
        raise ValueError(f"patch_dropout must be in [0, 1), got {rate}")
    return rate


def keep_count(P, rate):
    """Patches an image of P keeps at `rate`."""
    return max(1, int(P * (1.0 - check_rate(rate))))


def patch_bits(seed, sample_ids, P):
    """uint64 [B, P] holding the 32-bit bits_p of every image."""
    ids = np.asarray(list(sample_ids), dtype=np.int64).reshape(-1).astype(np.uint64) & _M32
    key = _fmix32((np.uint64(drop_key(seed, SITE)) + ids * np.uint64(0xB5297A4D)) & _M32)
    p = np.arange(P, dtype=np.uint64)
    return _fmix32((p[None, :] * np.uint64(0x9E3779B1) + key[:, None]) & _M32)


def keep_indices(seed, sample_ids, P, K):
    """-> (keep int32 [B, K] ascending, slot int32 [B, P]) for the images drawing under `sample_ids` (module docstring)."""
    P, K = int(P), int(K)
    if not 1 <= K <= P:
        raise ValueError(f"patch_dropout keeps K={K} patches, which must be in 1 .. P={P}")
    bits = patch_bits(seed, sample_ids, P)
    keep = np.sort(np.argsort(bits, axis=1, kind="stable")[:, :K], axis=1).astype(np.int32)
    slot = np.full(bits.shape, -1, dtype=np.int32)
    rows = np.arange(bits.shape[0])[:, None]
    slot[rows, keep] = np.arange(K, dtype=np.int32)[None, :]
    return keep, slot


class PatchDropSeeds(DropSeeds):
    """Patch dropout's private seed stream: DropSeeds' derivation from (base seed, rank) under another additive constant."""
    ADD = 0xA0761D6478BD642F
