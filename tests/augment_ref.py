"""CPU reference of `mmg_patchify_aug` (csrc/pixel_input.hip): the issue's arithmetic in torch fp32 (IEEE division, no contraction), from an
int32 copy of integer pixels.  What tests/test_pixel_input_gpu.py compares the kernel against, bit for bit; tests/test_augment_cpu.py checks it
against itself and against the formula of test_patchify_matches_conv_unfold.  Same role as tests/dwconv_ref.py.

Per image i, channel c and canvas pixel (y, x):
    ys = y - ty, xs = x - tx, inside = 0 <= ys < H and 0 <= xs < W;  flags & 2: ys = H-1-ys;  flags & 1: xs = W-1-xs     (flip over the FULL H, W)
    r = inside ? img[i, c, ys, xs] : 0;   x01 = r (fp32) | float(r) / 65535 (uint16) | float(r) / 255 (uint8)
    tone and (gain, offset) != (1, 0):  x01 = min(max(gain * x01 + offset, 0), 1)          (mul, then add; fill pixels included)
    v = scale16 ? (x01 * 65535 - 32767.5) / 32767.5 : x01
`augmented_images` returns x01 (what an un-augmented fp32 tower would have to be fed), `patch_rows` the bf16 rows of the stem."""
import torch

KIND_DIV = {torch.float32: None, torch.uint16: 65535.0, torch.uint8: 255.0}


def unit_pixels(img):
    """[..] fp32 / uint16 / uint8 -> fp32 x01 before any tone: r, float(r) / 65535, float(r) / 255 (integers through an int32 copy)."""
    div = KIND_DIV[img.dtype]
    if div is None:
        return img.clone()
    return img.to(torch.int32).to(torch.float32) / torch.tensor(div, dtype=torch.float32)


def gather(img, geom):
    """img [n, C, H, W] (any dtype torch can index; uint16 goes through int32) -> the flipped / shifted canvas [n, C, H, W], fill 0,
    in int32 for integer input and fp32 otherwise.  geom: n rows (flags, ty, tx, 0) or None."""
    src = img.to(torch.int32) if img.dtype in (torch.uint16, torch.uint8) else img
    n, C, H, W = src.shape
    if geom is None:
        return src.clone()
    out = torch.zeros_like(src)
    y, x = torch.arange(H), torch.arange(W)
    for i, (flags, ty, tx, _) in enumerate(geom):
        ys, xs = y - int(ty), x - int(tx)
        yin, xin = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
        if flags & 2:
            ys = H - 1 - ys
        if flags & 1:
            xs = W - 1 - xs
        picked = src[i][:, ys.clamp(0, H - 1)][:, :, xs.clamp(0, W - 1)]
        out[i] = torch.where((yin[:, None] & xin[None, :])[None], picked, torch.zeros_like(picked))
    return out


def augmented_images(img, geom=None, tone=None):
    """-> fp32 [n, C, H, W]: x01 after flip, shift, fill and tone - the pixels in [0, 1] that the plain fp32 path would have to be given."""
    div = KIND_DIV[img.dtype]
    g = gather(img, geom)
    x01 = g.clone() if div is None else g.to(torch.float32) / torch.tensor(div, dtype=torch.float32)
    if tone is not None:
        for i, (gain, offset) in enumerate(tone):
            gain, offset = torch.tensor(gain, dtype=torch.float32), torch.tensor(offset, dtype=torch.float32)
            if not (float(gain) == 1.0 and float(offset) == 0.0):
                x01[i] = torch.clamp(gain * x01[i] + offset, 0.0, 1.0)
    return x01


def scale(x01, scale16):
    return (x01 * 65535.0 - 32767.5) / 32767.5 if scale16 else x01


def rows_of(v, P, Kp):
    """fp32 [n, C, H, W] -> bf16 [n * (H // P) * (W // P), Kp]: rows (n, ho, wo), columns (kh, kw, ci), zero-padded; H // P, W // P floored."""
    n, C, H, W = v.shape
    Ho, Wo = H // P, W // P
    v = v[:, :, :Ho * P, :Wo * P].reshape(n, C, Ho, P, Wo, P).permute(0, 2, 4, 3, 5, 1).reshape(n * Ho * Wo, P * P * C)
    out = torch.zeros(n * Ho * Wo, Kp, dtype=torch.bfloat16)
    out[:, :P * P * C] = v.to(torch.bfloat16)
    return out


def patch_rows(img, P, Kp, scale16, geom=None, tone=None):
    return rows_of(scale(augmented_images(img, geom, tone), scale16), P, Kp)
