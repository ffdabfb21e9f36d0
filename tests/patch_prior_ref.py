"""CPU reference of the foreground prior of the ViT tower's patch dropout: the count of `mmg_patch_foreground` in torch fp32 on the CPU, on
the canvas that tests/augment_ref.py builds with `mmg_patchify_aug`'s geometry (flip over the full H, W -> shift -> fill 0), and the draw
through mmgclip.patch_dropout.keep_indices_prior, the numpy statement of record, re-exported here.  Same role as tests/patch_dropout_ref.py.

A canvas element is foreground iff inside && x01 > threshold, x01 = r | float(r) / 65535 | float(r) / 255 in fp32 (IEEE division), before any
tone.  The fill is raw 0, so x01 = 0 there, and the threshold is >= 0: `inside` needs no mask of its own.  NaN > t is false."""
import numpy as np
import torch

from mmgclip.patch_dropout import foreground_counts as numpy_counts, keep_count, keep_indices, keep_indices_prior  # noqa: F401
from tests import augment_ref as AR


def canvas01(img, geom=None):
    """img [n, C, H, W] fp32 / uint16 / uint8 -> fp32 [n, C, H, W]: x01 after flip, shift and fill, before any tone."""
    return AR.augmented_images(img, geom, None)


def foreground_counts(img, patch, threshold, geom=None):
    """-> int32 tensor [n, (H // patch) * (W // patch)]: per patch the canvas elements with x01 > fp32(threshold), over Cin * patch * patch
    elements; rows and columns beyond the last whole patch are ignored."""
    x = canvas01(img, geom)
    n, C, H, W = x.shape
    Ho, Wo = H // patch, W // patch
    fg = x[:, :, :Ho * patch, :Wo * patch] > torch.tensor(threshold, dtype=torch.float32)
    return fg.reshape(n, C, Ho, patch, Wo, patch).sum(dim=(1, 3, 5)).reshape(n, Ho * Wo).to(torch.int32)


def draw(seed, sample_ids, counts, min_pixels, K):
    """keep_indices_prior on a counts tensor or array -> (keep, slot, n_foreground) as int32 tensors."""
    keep, slot, nfg = keep_indices_prior(seed, sample_ids, np.asarray(counts), min_pixels, K)
    return torch.from_numpy(keep), torch.from_numpy(slot), torch.from_numpy(nfg)
