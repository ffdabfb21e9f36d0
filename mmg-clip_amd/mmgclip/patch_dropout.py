"""Patch dropout of the ViT tower (FLIP, Li et al. 2023; open_clip's `patch_dropout`) - decided here, on the host, as plain values, in the
style of networks/convnext_sd.py and augment.py.  Under train() every image keeps K of its P patches plus the class token; the encoder runs
on 1 + K tokens; eval() sees every patch.  The device makes the same draw in `mmg_patch_keep_indices` (csrc/patch_dropout.hip); this module
is the statement of record and what the tests compare that kernel against.

  * `check_rate`     rate in [0, 1), else ValueError.
  * `keep_count`     K = max(1, int(P * (1.0 - rate))): open_clip's rule, in Python doubles.  Every image keeps the same K (rectangular shapes).
  * `keep_indices`   (seed, sample_ids, P, K) -> (keep int32 [B, K], slot int32 [B, P]).
  * `PatchDropSeeds` one seed per forward that drops, a DropSeeds stream with an additive constant of its own (unrelated to the augmentation's,
                     to stochastic depth's and to the text tower's dropout), restarted from (base seed, rank) by `seeding(s)`.
  * `foreground_counts`, `keep_indices_prior`, `check_prior` / `check_threshold` / `check_min_pixels` / `check_dropout_eval`
                     the foreground prior (below, "the foreground prior"): the same K, drawn tissue first; `mmg_patch_foreground` and
                     `mmg_patch_keep_indices_prior` on the device.

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


# ---- the foreground prior --------------------------------------------------------------------------------------------------------------
# A mammogram is a breast on a black field, and a uniform draw spends much of its K tokens on that field.  Under patch_prior = "foreground"
# an image keeps its K patches foreground first: the key of patch p becomes (0 if foreground else 1, bits_p) - every patch that shows tissue
# before any patch that shows none, the hash above inside each class.  K, the [B, 1 + K] shapes and everything after the draw are unchanged.
#   counts[b, p]  = the canvas elements of patch p (Cin * patch * patch of them, after the augmentation's flip / shift / fill and BEFORE its
#                   tone) with x01 > patch_threshold                                  (`foreground_counts`; mmg_patch_foreground on the device)
#   foreground    iff counts[b, p] >= patch_min_pixels
# The selection is a function of (seed, sample id, the image's pixels, its geometry row), so it can also be made under eval() with a fixed
# seed and sample id (patch_dropout_eval): an image's embedding is then a function of its pixels alone.
PRIORS = ("uniform", "foreground")


def check_prior(prior):
    if not isinstance(prior, str) or prior not in PRIORS:
        raise ValueError(f"patch_prior must be one of {PRIORS}, got {prior!r}")
    return prior


def check_threshold(threshold):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise ValueError(f"patch_threshold must be a number in [0, 1), got {threshold!r}")
    threshold = float(threshold)
    if not 0.0 <= threshold < 1.0:      # (NaN and the infinities fail)
        raise ValueError(f"patch_threshold must be in [0, 1), got {threshold}")
    return threshold


def check_min_pixels(min_pixels, patch_elements):
    """patch_elements: Cin * patch * patch, the most a patch can count."""
    if isinstance(min_pixels, bool) or not isinstance(min_pixels, (int, np.integer)):
        raise ValueError(f"patch_min_pixels must be an int in 1 .. {patch_elements}, got {min_pixels!r}")
    if not 1 <= int(min_pixels) <= int(patch_elements):
        raise ValueError(f"patch_min_pixels must be in 1 .. {patch_elements} (Cin * patch^2), got {min_pixels}")
    return int(min_pixels)


def check_dropout_eval(flag, prior):
    if not isinstance(flag, (bool, np.bool_)):
        raise ValueError(f"patch_dropout_eval must be a bool, got {flag!r}")
    if flag and check_prior(prior) != "foreground":
        raise ValueError(f"patch_dropout_eval needs patch_prior='foreground': only a draw that is a function of the pixels can be repeated "
                         f"under eval(), got patch_prior={prior!r}")
    return bool(flag)


def foreground_counts(canvas01, patch, threshold):
    """canvas01: float32 [n, Cin, H, W], the canvas in [0, 1] as patchify forms it before the tone (flipped, shifted, fill 0).
    -> int32 [n, (H // patch) * (W // patch)]: per patch the elements > float32(threshold), summed over its Cin * patch * patch elements;
    rows and columns beyond the last whole patch are ignored.  (A fill pixel is 0 and threshold >= 0; NaN > t is false: both background.)"""
    x = np.asarray(canvas01, dtype=np.float32)
    n, C, H, W = x.shape
    Ho, Wo = H // patch, W // patch
    fg = x[:, :, :Ho * patch, :Wo * patch] > np.float32(check_threshold(threshold))
    return fg.reshape(n, C, Ho, patch, Wo, patch).sum(axis=(1, 3, 5)).reshape(n, Ho * Wo).astype(np.int32)


def keep_indices_prior(seed, sample_ids, counts, min_pixels, K):
    """-> (keep int32 [B, K] ascending, slot int32 [B, NP], n_foreground int32 [B]): image b keeps the K patches smallest under
    (0 if counts[b, p] >= min_pixels else 1, bits_p).  A row whose patches all fall in one class is `keep_indices`' row."""
    counts = np.asarray(counts)
    B, NP = counts.shape
    K, min_pixels = int(K), int(min_pixels)
    if not 1 <= K <= NP:
        raise ValueError(f"patch_dropout keeps K={K} patches, which must be in 1 .. P={NP}")
    if min_pixels < 1:
        raise ValueError(f"patch_min_pixels must be at least 1, got {min_pixels}")
    fg = counts >= min_pixels
    key = patch_bits(seed, sample_ids, NP) | (np.uint64(1) << np.uint64(32)) * (~fg).astype(np.uint64)      # the class bit above the 32
    if key.shape[0] != B:
        raise ValueError(f"sample_ids names {key.shape[0]} images, counts holds {B}")
    keep = np.sort(np.argsort(key, axis=1, kind="stable")[:, :K], axis=1).astype(np.int32)
    slot = np.full((B, NP), -1, dtype=np.int32)
    slot[np.arange(B)[:, None], keep] = np.arange(K, dtype=np.int32)[None, :]
    return keep, slot, fg.sum(axis=1).astype(np.int32)


class PatchDropSeeds(DropSeeds):
    """Patch dropout's private seed stream: DropSeeds' derivation from (base seed, rank) under another additive constant."""
    ADD = 0xA0761D6478BD642F
