"""Float64 reference, exact-data regimes, derived error bars and a tile-by-tile emulation (with mutations) for the depthwise 7x7
kernels of csrc/dwconv7.hip and csrc/dwconv7_mfma.hip.

Imported by tests/test_dwconv_ref_cpu.py (no GPU: the table covers every template instantiation, the exactness preconditions hold on
the reference alone, the emulation is inside every bar and every mutation of it is caught) and by tests/test_dwconv_gpu.py (the kernels
against the same reference); tests/test_dwconv_plan_cpu.py holds the host layer's plans (csrc/dwconv_plan.hip) against plan_text, the
restatement of the launchers' arithmetic below.  Everything here runs on the CPU in float64.

Layout: x, dy, add, y [n, H, W, C]; taps w49 [49, C] tap-major (w49[kh * 7 + kw, c] = weight[c, 0, kh, kw]); bias [C].
    y[n, h, w, c] = bias[c] + sum_{kh, kw} w49[kh * 7 + kw, c] x[n, h + kh - 3, w + kw - 3, c]  (+ add),   zero outside the image
flip uses w49[48 - k] in the place of w49[k] (with x := dy that is the data gradient);  dw[k, c] += sum_{n, h, w} x[n, h + kh - 3,
w + kw - 3, c] dy[n, h, w, c],  dbias[c] += sum dy.

Three data regimes.
  integer   every operand a small integer (taps drawn independently per channel and tap), so every fp32 partial sum is an integer below
            2^24 in ANY order - through the MFMA accumulators, the shuffles, the LDS reduction and the atomics - and every output is
            an integer of at most 256, which bf16 holds.  Bar: zero (torch.equal).
  readout   Gaussian bf16 x and ONE tap of 1.0 per channel: the output is a zero-padded shift of x, full mantissas and still exact.
            Weight gradient: dy is a single 1.0 per image and channel, x lies on a 2^-6 grid below 4, so dw is an exact sum of n inputs.
            Bar: zero.
  gaussian  the only regime with rounding; the bars are conv_bar / K_DW below.

Out of scope: the non-temporal store path (outputs of 256 MB and more), which no case here reaches (every case is at most about 12 M
elements), and the 32-bit addressing limits of dw_check."""
import functools
import zlib
from typing import NamedTuple, Optional

import torch

BF = torch.bfloat16
F64 = torch.float64
U32 = 2.0 ** -24         # unit round-off of fp32
# forward / data gradient: |got - ref64| <= half_ulp_bf16(ref64) + K 2^-24 (sum |w||x| + |bias| + |add|).  Derived: at most 49 products,
# a bias and an add are fewer than 64 fp32 roundings (the gamma_n bound of a 51-term sum in any order).
K = 64.0
# weight gradient: |got - ref64| <= K_DW 2^-24 sum |x||dy| per element, an fp32 sum of n H W terms in an unknown order (lanes, shuffles,
# LDS, atomics).  Measured, not derived: the smallest power of two >= 4 x the worst ratio recorded on an MI355X over every gaussian
# weight-gradient case of CASES at K_DW = 1 (profiles/dwconv_measured_tolerances.jsonl, field dw_ratio_k1: 0.986 at 2 x 3 x 5 - a
# 30-term sum, where the last fp32 rounding alone is half of it - and 0.20 - 0.37 in the other five cases; 4 x 0.986 = 3.9; DESIGN.md "Depthwise 7x7
# kernels against float64").  Conditions checked on the CPU: K_DW <= the term count of the smallest gaussian case, and one dropped
# pixel still leaves the bar there.
K_DW = 4.0
DW_FILL, DB_FILL = 5.0, -3.0          # dw / dbias are accumulated into: the exact regimes pre-fill them with these (gaussian: zero,
                                      # as the trainer does - the bar has no term for a rounding at the magnitude of a fill)


def fills(case):
    return (0.0, 0.0) if case.regime == "gaussian" else (DW_FILL, DB_FILL)
TILE_W, MFMA_T, CB = 32, 16, 32       # VALU tiles are TH x 32 pixels, matrix-core tiles 16 x 16; a slab is 32 channels


class Case(NamedTuple):
    n: int
    H: int
    W: int
    C: int
    regime: str                    # integer | readout | gaussian
    op: str = "conv"               # conv (forward, or data gradient with flip) | wgrad
    mfma: int = 0                  # MMG_DWCONV_MFMA (conv only)
    rows2: Optional[int] = None    # MMG_DWCONV_ROWS2, None = unset
    th: Optional[int] = None       # MMG_DWCONV_TH
    gth: Optional[int] = None      # MMG_DWG_TH
    waves: Optional[int] = None    # MMG_DWM_WAVES
    flip: bool = False
    add: bool = False
    bias: bool = True              # conv: bias given; wgrad: dbias given

    @property
    def id(self):
        s = f"{self.op}-{self.n}x{self.H}x{self.W}x{self.C}-{self.regime}"
        if self.op == "conv":
            s += "-mfma" if self.mfma else "-valu"
            s += ("-flip" if self.flip else "") + ("-add" if self.add else "") + ("-bias" if self.bias else "")
        elif not self.bias:
            s += "-nodbias"
        for tag, v in (("r", self.rows2), ("th", self.th), ("gth", self.gth), ("w", self.waves)):
            if v is not None:
                s += f"-{tag}{v}"
        return s

    @property
    def env(self):
        """The five knobs: {name: value or None (unset)}."""
        return {"MMG_DWCONV_MFMA": self.mfma, "MMG_DWCONV_ROWS2": self.rows2, "MMG_DWCONV_TH": self.th, "MMG_DWG_TH": self.gth,
                "MMG_DWM_WAVES": self.waves}

    @property
    def data_key(self):
        """What the operands and the reference depend on (not the knobs): cases that share it share one reference."""
        tap_bf16 = bool(self.mfma) and self.regime == "gaussian"
        return (self.n, self.H, self.W, self.C, self.regime, self.op, self.flip, self.add, self.bias, tap_bf16)


def cdiv(a, b):
    return -(-a // b)


# ---- the launchers' arithmetic (csrc/dwconv7.hip, csrc/dwconv7_mfma.hip), restated ------------------------------------------------
def tile_hw(case):
    """(tile height, tile width) of the kernel a case launches."""
    if case.op == "conv":
        if case.mfma:
            return MFMA_T, MFMA_T
        return (16 if case.rows2 != 0 and case.th == 16 else 8), TILE_W
    if case.rows2 == 0:
        return 8, TILE_W
    if case.gth in (8, 16):
        return case.gth, TILE_W
    return (16 if case.n * cdiv(case.H, 16) * cdiv(case.W, TILE_W) * (case.C // CB) >= 2048 else 8), TILE_W


def instantiations(case):
    """The kernel template instantiation a case launches."""
    th, _ = tile_hw(case)
    if case.op == "wgrad":
        return [("dwconv7_wgrad_kernel",) if case.rows2 == 0 else ("dwconv7_wgrad_rows2_kernel", th)]
    if case.mfma:
        return [("dwconv7_mfma_kernel", case.flip, 8 if case.waves == 8 else 16, case.add)]
    return [("dwconv7_kernel", case.flip) if case.rows2 == 0 else ("dwconv7_rows2_kernel", case.flip, th)]


def kernel_note(case):
    """mmg_last_kernel() after the case's launch (the matrix-core dispatcher does not spell ADD)."""
    inst = instantiations(case)[0]
    args = inst[1:3] if case.op == "conv" and case.mfma else inst[1:]
    spell = [("true" if a else "false") if isinstance(a, bool) else str(a) for a in args]
    return inst[0] + ("<" + ", ".join(spell) + ">" if spell else "")


ALL_INSTANTIATIONS = (
    {("dwconv7_kernel", f) for f in (False, True)} | {("dwconv7_rows2_kernel", f, t) for f in (False, True) for t in (8, 16)}
    | {("dwconv7_mfma_kernel", f, nw, a) for f in (False, True) for nw in (8, 16) for a in (False, True)}
    | {("dwconv7_wgrad_kernel",)} | {("dwconv7_wgrad_rows2_kernel", t) for t in (8, 16)})


def mfma_plan(n, H, W, C, cus):
    """mmg_dwconv7_nhwc_mfma's grid and dwconv7_mfma_kernel's deal of the (image, tile) items over its streams (workgroups)."""
    tiles_w, tiles_h = cdiv(W, MFMA_T), cdiv(H, MFMA_T)
    per_img, slabs = tiles_w * tiles_h, C // CB
    items = n * per_img
    per_xcd = max(cus // 8, slabs)
    want = cdiv(items, 8) * slabs
    if per_xcd > want:
        per_xcd = max(want, slabs)
    by_image = n >= 8
    counts, strides, slab_items = [], set(), [0] * slabs
    for b in range(8 * per_xcd):
        xcd, j = b & 7, b >> 3
        slab, u = j % slabs, j // slabs
        ns = (per_xcd - slab + slabs - 1) // slabs
        if by_image:
            seq, first, step = cdiv(n - xcd, 8) * per_img if n > xcd else 0, u, ns
        else:
            seq, first, step = items, u * 8 + xcd, 8 * ns
        counts.append(len(range(first, seq, step)))
        slab_items[slab] += counts[-1]
        strides.add(step)
    return dict(tiles_w=tiles_w, tiles_h=tiles_h, per_img=per_img, items=items, slabs=slabs, grid=8 * per_xcd, by_image=by_image,
                min_items=min(counts), max_items=max(counts), strides=strides, slab_items=slab_items)


def mfma_halo_paths(H, W):
    """{True, False}: whether some 16 x 16 tile's whole halo lies inside the image / some tile's does not (the uniform test of
    `request`: y0 >= 3 && x0 >= 3 && y0 + 19 <= H && x0 + 19 <= W)."""
    return {y0 >= 3 and x0 >= 3 and y0 + MFMA_T + 3 <= H and x0 + MFMA_T + 3 <= W
            for y0 in range(0, H, MFMA_T) for x0 in range(0, W, MFMA_T)}


def wgrad_plan(case, align=True):
    """mmg_dwconv7_wgrad's grid: per_slab workgroups walk the n * tiles items of a slab with a grid stride.  align: MMG_DWG_ALIGN."""
    th, tw = tile_hw(case)
    tiles, slabs = cdiv(case.W, tw) * cdiv(case.H, th), case.C // CB
    per_slab = 1024 // slabs
    if align and per_slab >= 8:
        per_slab &= ~7
    per_slab = max(per_slab, 1)
    capped = per_slab > case.n * tiles
    per_slab = min(per_slab, case.n * tiles)
    return dict(TH=th, tiles=tiles, items=case.n * tiles, per_slab=per_slab, capped=capped, min_items=case.n * tiles // per_slab,
                max_items=cdiv(case.n * tiles, per_slab))


# Dynamic LDS, from the launchers before the host layer csrc/dwconv_plan.hip.  VALU kernels: the staged halo tile, rows of 38 columns x 16
# channel pairs (dwords) padded by 16 dwords in the one-row kernels ([8 + 6] rows) and by 8 in the two-row kernels ([TH + 6] rows); behind
# it the slab's taps [49][32] fp32 (forward) or the reduction buffer [4 waves][50][32] fp32 (weight gradient).  Matrix cores: the NHWC halo
# tile (2048 chunks of 16 bytes), 32 channel planes of 22 rows x 96 bytes + 16, the NHWC output tile (16 x 16 pixels x 80 bytes) - and a
# second output tile for the low halves of the accumulators when `add` is given.
ROWD, ROWD2 = 38 * 16 + 16, 38 * 16 + 8
MFMA_LDS = 2048 * 16 + 32 * (22 * 96 + 16) + 16 * 16 * 80
MFMA_LDS_ADD = MFMA_LDS + 16 * 16 * 80
NT_BYTES = 256 << 20              # outputs of this many bytes and more are stored past L2


def lds(case):
    """Dynamic LDS bytes of the case's launch."""
    if case.op == "conv" and case.mfma:
        return MFMA_LDS_ADD if case.add else MFMA_LDS
    th, _ = tile_hw(case)
    tile = (14 * ROWD if case.rows2 == 0 else (th + 6) * ROWD2) * 4
    return tile + (49 * CB * 4 if case.op == "conv" else 4 * 50 * CB * 4)


def block(case):
    """Threads per workgroup: the VALU kernels 256, the matrix-core kernel 64 per wave."""
    return 64 * (8 if case.waves == 8 else 16) if case.op == "conv" and case.mfma else 256


def nt(case):
    """Streaming stores: an output of 256 MiB and more (the weight gradient has no such output)."""
    return int(case.op == "conv" and case.n * case.H * case.W * case.C * 2 >= NT_BYTES)


def grid(case, cus, align=True):
    """(x, y, z) of the case's launch on a device of `cus` CUs (only the matrix-core kernel reads them)."""
    th, tw = tile_hw(case)
    if case.op == "wgrad":
        return wgrad_plan(case, align)["per_slab"], case.C // CB, 1
    if case.mfma:
        return mfma_plan(case.n, case.H, case.W, case.C, cus)["grid"], 1, 1
    return cdiv(case.W, tw) * cdiv(case.H, th), case.C // CB, case.n


def plan_args(case, cus):
    """The arguments of mmg_dwconv7_plan for the case."""
    op = 2 if case.op == "wgrad" else (1 if case.mfma else 0)
    return op, case.n, case.H, case.W, case.C, int(case.flip and op != 2), int(case.add and op != 2), cus


def plan_text(case, cus, align=True):
    """What mmg_dwconv7_plan returns for the case on a device of `cus` CUs."""
    th, tw = tile_hw(case)
    x, y, z = grid(case, cus, align)
    text = (f"{kernel_note(case)} grid=({x},{y},{z}) block={block(case)} lds={lds(case)} nt={nt(case)} tile={th}x{tw} "
            f"items={case.n * cdiv(case.H, th) * cdiv(case.W, tw)}")
    if case.op == "conv" and case.mfma:
        text += f" add={int(case.add)} by_image={int(case.n >= 8)}"
    return text


# ---- the table -------------------------------------------------------------------------------------------------------------------
def _table():
    T = []

    def conv(shape, regime, mfma, flip=False, add=False, bias=True, **kw):
        if regime == "readout":
            add, bias = False, False
        T.append(Case(*shape, regime, "conv", mfma, flip=flip, add=add, bias=bias, **kw))

    def wg(shape, regime, bias=True, **kw):
        T.append(Case(*shape, regime, "wgrad", bias=bias, **kw))

    # --- degenerate maps.  1 x 1: every halo pixel but the centre lies outside the image, every tile is partial
    s = (1, 1, 1, 32)
    conv(s, "integer", 0)
    conv(s, "integer", 0, flip=True, add=True, bias=False, rows2=0)
    conv(s, "integer", 1, add=True)
    conv(s, "integer", 1, flip=True, bias=False, waves=8)
    wg(s, "integer")
    wg(s, "integer", bias=False, rows2=0)
    # 3 x 5: smaller than the 7 x 7 kernel in both directions (taps that never meet data); C = 64 >= 49: every tap is read out
    s = (2, 3, 5, 64)
    conv(s, "integer", 0, flip=True, add=True, th=16)
    conv(s, "integer", 1, flip=True, add=True, waves=8)
    conv(s, "readout", 0)
    conv(s, "readout", 1, flip=True)
    conv(s, "gaussian", 0, add=True)
    conv(s, "gaussian", 1)
    wg(s, "integer", gth=16)
    wg(s, "readout")
    wg(s, "gaussian")                      # the smallest gaussian weight-gradient case: 2 x 3 x 5 = 30 terms per element
    # 7 x 7: exactly the kernel; C = 96: three slabs
    s = (1, 7, 7, 96)
    conv(s, "integer", 0, add=True)                          # add without flip on the VALU kernels
    conv(s, "integer", 1, add=True, waves=8)                 # ADD with FLIP = false on the matrix cores
    conv(s, "readout", 0, flip=True, rows2=0)
    conv(s, "readout", 1, waves=8)
    wg(s, "integer")
    wg(s, "readout", rows2=0)
    # --- exact tiles, and one pixel over.  VALU 8 x 32: cdiv(8, 8) x cdiv(32, 32) = 1 tile, 9 x 33 -> 2 x 2 tiles of which three partial
    s = (2, 8, 32, 32)
    conv(s, "integer", 0, th=8)
    conv(s, "integer", 0, flip=True, add=True, rows2=0)
    wg(s, "integer", gth=8)
    s = (1, 9, 33, 64)
    conv(s, "integer", 0, flip=True, th=8)
    conv(s, "integer", 0, add=True, bias=False, rows2=0)
    conv(s, "readout", 0, rows2=0)
    conv(s, "gaussian", 0, flip=True, add=True)
    wg(s, "integer", rows2=0)
    wg(s, "readout", gth=8)
    # TH = 16: 16 x 32 = 1 tile in two passes, 17 x 33 -> 2 x 2 tiles, the second tile row holding ONE image row (pass 1 all masked)
    s = (2, 16, 32, 32)
    conv(s, "integer", 0, add=True, th=16)
    conv(s, "integer", 0, flip=True, th=16)
    wg(s, "integer", gth=16)
    s = (1, 17, 33, 32)
    conv(s, "integer", 0, flip=True, add=True, th=16)
    conv(s, "integer", 0, bias=False, th=16)
    wg(s, "integer", gth=16)
    wg(s, "gaussian", gth=16)
    # matrix cores 16 x 16: 1 tile per image (per_img = 1: the quotient by per_img is skipped), 17 x 17 -> 2 x 2 tiles
    s = (2, 16, 16, 32)
    conv(s, "integer", 1)
    conv(s, "integer", 1, flip=True, add=True, waves=8)
    s = (1, 17, 17, 64)
    conv(s, "integer", 1, flip=True)                         # FLIP without ADD on the matrix cores
    conv(s, "integer", 1, add=True, waves=8)
    conv(s, "readout", 1)
    conv(s, "gaussian", 1)
    # --- interior and edge tiles in one launch.  37 x 50, three slabs: VALU 5 x 2 (TH 8) / 3 x 2 (TH 16) tiles, the right and the bottom
    # ones partial; matrix cores 3 x 4 tiles, ONE with its whole halo inside the image (y0 = x0 = 16: 16 + 19 = 35 <= 37, 50)
    s = (3, 37, 50, 96)
    conv(s, "integer", 0)
    conv(s, "integer", 0, add=True, rows2=0)
    conv(s, "integer", 0, flip=True, add=True, th=16)
    conv(s, "integer", 1, flip=True, add=True)
    conv(s, "integer", 1, waves=8)
    conv(s, "readout", 0, flip=True, th=16)
    conv(s, "readout", 0)
    conv(s, "readout", 1, flip=True, waves=8)
    conv(s, "readout", 1)
    conv(s, "gaussian", 0)
    conv(s, "gaussian", 0, flip=True, add=True, rows2=0)
    conv(s, "gaussian", 1)
    conv(s, "gaussian", 1, flip=True, add=True)              # the tower's data-gradient call on large maps
    wg(s, "integer")
    wg(s, "readout", gth=16)
    wg(s, "gaussian", rows2=0)
    wg(s, "gaussian", gth=8)
    wg(s, "gaussian", gth=16)
    # 64 x 70: 4 x 5 matrix-core tiles; those at y0 in (16, 32), x0 in (16, 32, 48) have y0 + 19 <= 64 and x0 + 19 <= 70: halo inside
    s = (1, 64, 70, 32)
    conv(s, "integer", 1, add=True)
    conv(s, "integer", 1, flip=True, waves=8)
    conv(s, "integer", 0, th=16)
    conv(s, "gaussian", 1, bias=True, waves=8)
    # --- by-image walk: n = 9 >= 8 and 9 % 8 != 0 - XCD group 0 owns images 0 and 8, the others one image; 2 x 3 tiles per image
    s = (9, 20, 35, 32)
    conv(s, "integer", 1, flip=True, add=True)
    conv(s, "integer", 1, waves=8)
    conv(s, "integer", 0)
    conv(s, "gaussian", 1, flip=True)
    # --- matrix-core item loop at n < 8 (on 256 CUs; test_dwconv_gpu asserts the figure from mmg_device_cu_count()).
    # 250 x 270: 16 x 17 = 272 tiles, 5 x 272 = 1360 items, 1 slab -> 256 streams of stride 256: 5 or 6 items each; 272 % 256 = 16
    conv((5, 250, 270, 32), "integer", 1, flip=True, add=True)
    # 170 x 180: 11 x 12 = 132 tiles, 396 items; 4 slabs -> 64 streams per slab, stride 64: 6 or 7 items each; 132 % 64 = 4
    conv((3, 170, 180, 128), "integer", 1, waves=8)
    # --- weight-gradient item loop.  C = 1024: 32 slabs, per_slab = 1024 / 32 = 32 workgroups.  9 x 97 at TH = 8: 2 x 4 = 8 tiles,
    # 12 x 8 = 96 items = 3 per workgroup; at TH = 16: 1 x 4 tiles, 48 items = 1 or 2 per workgroup.  Unset: 12 x 1 x 4 x 32 = 1536 < 2048 -> 8
    s = (12, 9, 97, 1024)
    wg(s, "integer", gth=8)
    wg(s, "integer", gth=16)
    wg(s, "integer")
    wg(s, "integer", rows2=0)
    # TH = 16 with three items per workgroup (the barrier of pass 0 between items): 17 x 9 -> 2 x 1 tiles, 48 x 2 = 96 items over 32
    wg((48, 17, 9, 1024), "integer", gth=16)
    # per_slab capped by the item count: 2 slabs -> 512 workgroups per slab, but 2 x (2 x 2 tiles) = 8 items: 8 workgroups, one item each
    wg((2, 9, 33, 64), "integer")
    # gaussian through the item loop: 64 slabs -> 16 workgroups per slab; 9 x 33 at TH = 8: 2 x 2 tiles, 12 x 4 = 48 items = 3 each
    wg((12, 9, 33, 2048), "gaussian")
    return T


CASES = _table()


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _rb(x):
    """Round to bf16, back in float64."""
    return x.to(torch.float32).to(BF).to(F64)


def half_ulp_bf16(v):
    """Half the spacing of bf16 numbers at |v| (float64 in and out); the smallest normal's below that."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 9)


def readout_tap(c):
    """The single tap of channel c in the read-out regime: 7 c + c // 7 (mod 49) visits every tap once per 49 channels."""
    return (7 * c + c // 7) % 49


def readout_pixels(H, W):
    """Pixels of the weight-gradient read-out, taken in turn by the channels: the four corners, both sides of the tile seams of every
    tile height (rows 7 | 8 and 15 | 16, columns 31 | 32), the first pixel of the last partial tile."""
    P = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (7, 31), (8, 32), (15, 31), (16, 32), ((H - 1) // 16 * 16, (W - 1) // 32 * 32)]
    return [(min(h, H - 1), min(w, W - 1)) for h, w in P]


def make_data(case):
    """dict of float64 tensors holding bf16-exact x / dy / add and fp32-exact w49 / bias."""
    n, H, W, C = case.n, case.H, case.W, case.C
    g = torch.Generator().manual_seed(zlib.crc32(repr(case.data_key).encode()))
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    d = dict(w49=None, bias=None, add=None, dy=None)
    if case.op == "conv":
        if case.regime == "integer":           # |y| <= 49 * 2 * 2 + 16 + 16 = 228
            d.update(x=ri(-2, 2, n, H, W, C), w49=ri(-2, 2, 49, C))
            d["bias"] = ri(-16, 16, C) if case.bias else None
            d["add"] = ri(-16, 16, n, H, W, C) if case.add else None
        elif case.regime == "readout":
            w = torch.zeros(49, C, dtype=F64)
            w[[readout_tap(c) for c in range(C)], torch.arange(C)] = 1.0
            d.update(x=_rb(torch.randn(n, H, W, C, generator=g, dtype=F64)), w49=w)
        else:
            w = (0.1 * torch.randn(49, C, generator=g, dtype=F64)).to(torch.float32)
            d.update(x=_rb(torch.randn(n, H, W, C, generator=g, dtype=F64)),
                     w49=(w.to(BF) if case.mfma else w).to(F64))       # the matrix cores multiply by bf16-rounded taps: their contract
            d["w49_f32"] = w                                             # what the kernel is given
            d["bias"] = torch.randn(C, generator=g, dtype=F64).to(torch.float32).to(F64) if case.bias else None
            d["add"] = _rb(torch.randn(n, H, W, C, generator=g, dtype=F64)) if case.add else None
    else:
        if case.regime == "integer":           # |dw| <= 4 n H W + 5, far below 2^24
            d.update(x=ri(-2, 2, n, H, W, C), dy=ri(-2, 2, n, H, W, C))
        elif case.regime == "readout":
            dy = torch.zeros(n, H, W, C, dtype=F64)
            P = readout_pixels(H, W)
            for c in range(C):
                h, w = P[c % len(P)]
                dy[:, h, w, c] = 1.0
            d.update(x=ri(-255, 255, n, H, W, C) / 64.0, dy=dy)
        else:
            d.update(x=_rb(torch.randn(n, H, W, C, generator=g, dtype=F64)), dy=_rb(torch.randn(n, H, W, C, generator=g, dtype=F64)))
    return d


# ---- float64 reference -----------------------------------------------------------------------------------------------------------
def _pad3(x):
    return torch.nn.functional.pad(x, (0, 0, 3, 3, 3, 3))


def conv64(x, w49, bias=None, add=None, flip=False):
    n, H, W, C = x.shape
    xp = _pad3(x)
    y = torch.zeros_like(x) if bias is None else bias.expand(n, H, W, C).clone()
    for k in range(49):
        kh, kw = divmod(k, 7)
        y.addcmul_(xp[:, kh:kh + H, kw:kw + W], w49[48 - k if flip else k])
    return y if add is None else y + add


def wgrad64(x, dy):
    n, H, W, C = x.shape
    xp = _pad3(x)
    dw = torch.stack([(xp[:, kh:kh + H, kw:kw + W] * dy).sum((0, 1, 2)) for kh in range(7) for kw in range(7)])
    return dw, dy.sum((0, 1, 2))


def reference(case, d):
    """conv: y (float64), pre (y before the add), mag (sum |w||x| + |bias| + |add|, gaussian only).
    wgrad: dw, dbias (including the pre-fill), dw_mag / db_mag (sum |x||dy|, sum |dy|, gaussian only)."""
    if case.op == "conv":
        pre = conv64(d["x"], d["w49"], d["bias"], None, case.flip)
        r = dict(pre=pre, y=pre if d["add"] is None else pre + d["add"])
        if case.regime == "gaussian":
            ab = lambda t: None if t is None else t.abs()
            r["mag"] = conv64(d["x"].abs(), d["w49"].abs(), ab(d["bias"]), ab(d["add"]), case.flip)
        return r
    dw, db = wgrad64(d["x"], d["dy"])
    r = dict(dw=dw + fills(case)[0], dbias=db + fills(case)[1])
    if case.regime == "gaussian":
        r["dw_mag"], r["db_mag"] = wgrad64(d["x"].abs(), d["dy"].abs())
    return r


@functools.lru_cache(maxsize=2)
def _prepared(key, case):
    d = make_data(case)
    return d, reference(case, d)


def prepared(case):
    """(data, float64 reference) of a case, computed once per data_key and shared (callers must not modify them)."""
    return _prepared(case.data_key, next((c for c in CASES if c.data_key == case.data_key), case))


# ---- preconditions of the exact regimes, on the reference alone ------------------------------------------------------------------
def exactness_violations(case, d, ref):
    """Why a bar of zero would NOT be justified for this integer / read-out case (empty list: it is)."""
    bad = []
    is_int = lambda t: bool((t == t.round()).all())
    if case.regime == "integer" and case.op == "conv":
        for name in ("pre", "y"):
            if not (is_int(ref[name]) and float(ref[name].abs().max()) <= 256):
                bad.append(f"{name} is not an integer of at most 256")
    elif case.regime == "integer":
        for name in ("dw", "dbias"):
            if not (is_int(ref[name]) and float(ref[name].abs().max()) < 2 ** 24):
                bad.append(f"{name} is not an integer below 2^24")
        aw, ab = wgrad64(d["x"].abs(), d["dy"].abs())
        if not float(aw.max()) + DW_FILL < 2 ** 24 or not float(ab.max()) + abs(DB_FILL) < 2 ** 24:
            bad.append("a partial sum could pass 2^24")
    elif case.op == "conv":
        if case.C < 49 or d["bias"] is not None or d["add"] is not None:
            bad.append("read-out needs C >= 49 (every tap once), no bias and no add")
        if len({readout_tap(c) for c in range(case.C)}) != 49:
            bad.append("not every tap is read out")
        xp = _pad3(d["x"])
        for c in range(case.C):
            k = readout_tap(c)
            kh, kw = divmod(48 - k if case.flip else k, 7)       # the kernel position at which tap k is applied
            if not torch.equal(ref["y"][..., c], xp[:, kh:kh + case.H, kw:kw + case.W, c]):
                bad.append(f"channel {c} is not the shift of x")
                break
        if not torch.equal(_rb(ref["y"]), ref["y"]):
            bad.append("y is not bf16-exact")
    else:
        x64 = d["x"] * 64
        if not (is_int(x64) and float(x64.abs().max()) < 256 and case.n * 256 < 2 ** 24):
            bad.append("x is not on the 2^-6 grid below 4")
        if not torch.equal(_rb(d["x"]), d["x"]):
            bad.append("x is not bf16-exact")
        if not bool((d["dy"].sum((1, 2)) == 1).all()) or not bool(((d["dy"] == 0) | (d["dy"] == 1)).all()):
            bad.append("dy is not a single 1.0 per image and channel")
        if not (is_int((ref["dw"] - DW_FILL) * 64) and torch.equal(ref["dbias"], torch.full_like(ref["dbias"], case.n + DB_FILL))):
            bad.append("dw is not a sum of n grid values / dbias is not n")
        if not torch.equal(ref["dw"].to(torch.float32).to(F64), ref["dw"]):
            bad.append("dw is not fp32-exact")
    return bad


# ---- bars ------------------------------------------------------------------------------------------------------------------------
def check_conv(case, ref, got, sel=None):
    """got (float64 holding bf16 values, [n, H, W, C]) against the reference -> (worst ratio to the bar, share of elements that differ
    from bf16(ref)).  Integer / read-out: the bar is zero, the ratio 0.0 (equal) or inf.  sel: (image, channel slice) to compare."""
    y = ref["y"]
    mag = ref.get("mag")
    if sel is not None:
        y = y[sel[0]:sel[0] + 1, ..., sel[1]]
        mag = None if mag is None else mag[sel[0]:sel[0] + 1, ..., sel[1]]
    differ = (got != _rb(y)).double().mean().item()
    if not torch.isfinite(got).all():
        return float("inf"), differ
    if case.regime != "gaussian":
        return (0.0 if differ == 0 else float("inf")), differ
    ratio = (got - y).abs() / (half_ulp_bf16(y) + K * U32 * mag)
    return ratio.max().item(), differ


def check_wgrad(case, ref, dw, dbias, sel=None, k_dw=None):
    """dw [49, C], dbias [C] or None (float64 holding fp32 values) -> {"dw": ratio, "dbias": ratio} at K_DW (or k_dw)."""
    k_dw = K_DW if k_dw is None else k_dw
    s = slice(None) if sel is None else sel
    out = {}
    for name, got, mag in (("dw", dw, "dw_mag"), ("dbias", dbias, "db_mag")):
        if got is None:
            continue
        r = ref[name][..., s]
        if not torch.isfinite(got).all():
            out[name] = float("inf")
        elif case.regime != "gaussian":
            out[name] = 0.0 if torch.equal(got, r) else float("inf")
        else:
            diff, bar = (got - r).abs(), k_dw * U32 * ref[mag][..., s]       # (a tap that never meets data: bar 0, dw must be the fill)
            out[name] = torch.where(diff == 0, torch.zeros_like(diff), diff / bar).max().item()
    return out


# ---- tile-by-tile emulation of the kernels, and mutations of it ------------------------------------------------------------------
# pre_add_round: the convolution rounded to bf16 BEFORE the residual operand is added and the sum rounded again (two roundings where the
# contract has one) - the smallest of them, a rounding-size error, and so required of the gaussian cases only
CONV_MUTATIONS = ("border_tap", "halo_shift", "replicate", "prev_mask", "no_flip", "swap_pair", "add_partial", "partial_row",
                  "skip_image", "udiv", "pre_add_round")
WGRAD_MUTATIONS = ("item_missing", "pass2_missing", "dbias_oob", "pixel_dropped")


def _tiles(case):
    th, tw = tile_hw(case)
    return [(h0, w0) for h0 in range(0, case.H, th) for w0 in range(0, case.W, tw)]


def _halo(xi, h0, w0, th, tw, mut=None, prev=None):
    """The (th + 6) x (tw + 6) halo tile of image xi [H, W, C] at tile origin (h0, w0): a clamped gather times the in-image mask."""
    H, W, _ = xi.shape
    rows = torch.arange(h0 - 3, h0 + th + 3)
    cols = torch.arange(w0 - 3, w0 + tw + 3) + (1 if mut == "halo_shift" else 0)
    halo = xi[rows.clamp(0, H - 1)][:, cols.clamp(0, W - 1)]
    if mut == "replicate":                       # the mask is lost: what the clamped addresses hold
        return halo

    def mask(a, b):
        r, c = torch.arange(a - 3, a + th + 3), torch.arange(b - 3, b + tw + 3) + (1 if mut == "halo_shift" else 0)
        return (((r >= 0) & (r < H))[:, None] & ((c >= 0) & (c < W))[None, :]).to(F64)

    m = mask(h0, w0)
    if mut == "prev_mask" and prev is not None:  # the mask of the previous item travels with this item's registers
        m = m * mask(*prev)
    return halo * m[..., None]


def mutation_applies(case, mut):
    """Whether the case contains the feature a mutation breaks."""
    th, tw = tile_hw(case)
    H, W = case.H, case.W
    partial = H % th != 0 or W % tw != 0
    return {
        "border_tap": H >= 4 and W >= 4,                 # tap 0 meets data
        "halo_shift": W >= 2,
        "replicate": H * W >= 2,                         # a clamped address holds another pixel than the centre
        "prev_mask": len(_tiles(case)) >= 2,
        "no_flip": case.flip and H * W >= 2,             # (on a 1 x 1 map only the centre tap, its own mirror image, meets data)
        "swap_pair": True,
        "add_partial": case.add and partial,
        "partial_row": H % th != 0,
        "skip_image": case.n >= 8 and bool(case.mfma),
        "udiv": cdiv(H, th) >= 2,
        "pre_add_round": case.add and case.regime == "gaussian",
        "item_missing": True,
        "pass2_missing": th == 16 and H > 8,
        "dbias_oob": case.bias and partial,
        "pixel_dropped": case.regime != "readout",      # (the read-out dy is zero at almost every pixel)
    }[mut]


def emulate_conv(case, d, mut=None):
    """float64 with the rounding points of the kernels' contract: the taps as the kernel multiplies them (d["w49"]: bf16 on the matrix
    cores) and the output to bf16, once.  Unmutated: every image and channel.
    mut: one of CONV_MUTATIONS, applied to image 0 (skip_image: the last image), slab 0; returns ([1, H, W, 32], (image, slice))."""
    th, tw = tile_hw(case)
    H, W = case.H, case.W
    img = case.n - 1 if mut == "skip_image" else 0
    imgs, ch = (range(case.n), slice(None)) if mut is None else ([img], slice(0, CB))
    x, w = d["x"][..., ch], d["w49"][:, ch]
    bias = None if d["bias"] is None else d["bias"][ch]
    add = None if d["add"] is None else d["add"][..., ch]
    if mut == "swap_pair":                       # the low and the high half of a packed bf16 pair exchanged on the way in
        x = x.reshape(*x.shape[:-1], -1, 2).flip(-1).reshape(x.shape)
    flip = case.flip and mut != "no_flip"
    wk = w.flip(0) if flip else w
    if mut == "border_tap":
        wk = wk.clone()
        wk[48 if flip else 0] = 0.0              # tap 0 of the weights never applied
    out = torch.zeros(len(imgs), H, W, x.shape[-1], dtype=F64)
    tiles = _tiles(case)
    for o, i in enumerate(imgs):
        if mut == "skip_image":
            continue
        for t, (h0, w0) in enumerate(tiles):
            if mut == "udiv" and w0 == 0 and h0 > 0:       # quotient one short at an exact multiple of tiles_w: the tile lands past the row
                continue
            halo = _halo(x[i], h0, w0, th, tw, mut, tiles[t - 1] if t else None)
            acc = torch.zeros(th, tw, x.shape[-1], dtype=F64) if bias is None else bias.expand(th, tw, -1).clone()
            for k in range(49):
                kh, kw = divmod(k, 7)
                acc.addcmul_(halo[kh:kh + th, kw:kw + tw], wk[k])
            hh, ww = min(th, H - h0), min(tw, W - w0)
            acc = acc[:hh, :ww]
            if add is not None and not (mut == "add_partial" and (hh < th or ww < tw)):
                acc = (_rb(acc) if mut == "pre_add_round" else acc) + add[i, h0:h0 + hh, w0:w0 + ww]
            if mut == "partial_row" and hh < th:
                hh -= 1
            out[o, h0:h0 + hh, w0:w0 + ww] = _rb(acc[:hh])
    return out if mut is None else (out, (img, ch))


def emulate_wgrad(case, d, mut=None):
    """Item by item (image, tile): the zero-padded halo tile times the masked dy tile, float64, rounded to fp32 at the end.
    Unmutated: every slab.  mut: one of WGRAD_MUTATIONS, applied to an item of image 0, slab 0; returns (dw, dbias, slice)."""
    th, tw = tile_hw(case)
    H, W = case.H, case.W
    ch = slice(None) if mut is None else slice(0, CB)
    x, dy = d["x"][..., ch], d["dy"][..., ch]
    Cc = x.shape[-1]
    dw, db = torch.full((49, Cc), fills(case)[0], dtype=F64), torch.full((Cc,), fills(case)[1], dtype=F64)
    tiles = _tiles(case)
    for i in range(case.n):
        for t, (h0, w0) in enumerate(tiles):
            hit = mut is not None and i == 0 and t == len(tiles) - 1
            if hit and mut == "item_missing":
                continue
            halo = _halo(x[i], h0, w0, th, tw)
            hh, ww = min(th, H - h0), min(tw, W - w0)
            g = torch.zeros(th, tw, Cc, dtype=F64)
            g[:hh, :ww] = dy[i, h0:h0 + hh, w0:w0 + ww]
            if mut == "pass2_missing" and i == 0 and t == 0:
                g[8:] = 0.0
            if mut == "pixel_dropped" and i == 0 and t == 0:
                g[min(hh, 8) // 2, min(ww, 8) // 2] = 0.0
            db += g.sum((0, 1))
            if hit and mut == "dbias_oob":           # the bounds test lost: the clamped addresses' dy counted as well
                r, c = torch.arange(h0, h0 + th).clamp(max=H - 1), torch.arange(w0, w0 + tw).clamp(max=W - 1)
                db += dy[i][r][:, c].sum((0, 1)) - g.sum((0, 1))
            for k in range(49):
                kh, kw = divmod(k, 7)
                dw[k] += (halo[kh:kh + th, kw:kw + tw] * g).sum((0, 1))
    dw, db = dw.to(torch.float32).to(F64), db.to(torch.float32).to(F64)
    return (dw, db if case.bias else None) if mut is None else (dw, db if case.bias else None, ch)
