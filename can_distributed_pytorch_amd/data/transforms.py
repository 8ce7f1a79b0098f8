"""Image/density-map transforms with the reference's exact semantics, without OpenCV.

The reference resizes with cv2.resize(..., INTER_LINEAR) (model/CrowdDataset.py:57-61):
half-pixel-centre bilinear interpolation, source coordinates clamped to the
border, NO anti-aliasing when shrinking (the 1/8 density map is point-sampled
between pixels 8x+3 and 8x+4, then multiplied by 64).  ``resize_linear`` is a
separable float64 implementation of that rule (cv2 computes float images in
float arithmetic, so this matches it to rounding).
"""
from __future__ import annotations

import numpy as np

IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def _axis_weights(in_size: int, out_size: int):
    scale = in_size / out_size
    src = (np.arange(out_size, dtype=np.float64) + 0.5) * scale - 0.5
    x0 = np.floor(src)
    frac = src - x0
    x0 = x0.astype(np.int64)
    # cv2 border handling: clamp both taps into [0, in-1]; a coordinate left
    # of 0 collapses onto pixel 0 (weight moves entirely to the clamped tap)
    neg = x0 < 0
    frac[neg] = 0.0
    x0[neg] = 0
    x1 = np.minimum(x0 + 1, in_size - 1)
    x0 = np.minimum(x0, in_size - 1)
    return x0, x1, frac


def resize_linear(arr: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """cv2.resize(arr, (out_w, out_h), interpolation=INTER_LINEAR) for HxW or HxWxC float arrays."""
    h, w = arr.shape[:2]
    if (h, w) == (out_h, out_w):
        return arr.copy()
    a = arr.astype(np.float64, copy=False)
    y0, y1, fy = _axis_weights(h, out_h)
    x0, x1, fx = _axis_weights(w, out_w)
    shape_y = (-1,) + (1,) * (a.ndim - 1)
    rows = a[y0] * (1.0 - fy).reshape(shape_y) + a[y1] * fy.reshape(shape_y)
    shape_x = (1, -1) + (1,) * (a.ndim - 2)
    out = rows[:, x0] * (1.0 - fx).reshape(shape_x) + rows[:, x1] * fx.reshape(shape_x)
    return out.astype(arr.dtype if arr.dtype.kind == "f" else np.float64)


def to_unit_float(img: np.ndarray) -> np.ndarray:
    """Integer images /255 -> [0,1]; float images are kept (reference Q14: PNGs are already float)."""
    if img.dtype.kind in "ui":
        return img.astype(np.float64) / 255.0
    return img.astype(np.float64)


def gray_to_rgb(img: np.ndarray) -> np.ndarray:
    if img.ndim == 2:
        img = img[:, :, None]
    if img.shape[2] == 1:
        img = np.concatenate([img, img, img], axis=2)
    if img.shape[2] == 4:  # RGBA -> RGB
        img = img[:, :, :3]
    return img


GRAY_MIX = np.array([0.299, 0.587, 0.114], dtype=np.float32)        # luma weights of (r, g, b), float32 as on the GPU


def photo_table(b: float, c: float, g: float) -> np.ndarray:
    """The tone table float32 [256] of a photometric draw (brightness shift b, contrast factor c about mid-gray, gamma
    g), on the 0..255 scale: t = (u/255)^g, t = clip(c (t - 0.5) + 0.5 + b, 0, 1), table[u] = float32(255 t), in
    float64.  The GPU kernel sees only this table, so both paths share it bit for bit; photo_table(0, 1, 1) is
    arange(256) exactly."""
    t = (np.arange(256, dtype=np.float64) / 255.0) ** float(g)
    t = np.minimum(1.0, np.maximum(0.0, float(c) * (t - 0.5) + 0.5 + float(b)))
    return (255.0 * t).astype(np.float32)


def apply_photo(img_u8: np.ndarray, table: np.ndarray, gray: bool) -> np.ndarray:
    """The photometric jitter of a uint8 image [H, W] / [H, W, 1 | 3 | 4] -> float64 [H, W, 3] in [0, 1]: every byte
    through the tone table, with ``gray`` a colour pixel's three channels replaced by their luma (GRAY_MIX, summed in
    float64 in the kernel's order; a 1-channel image is left alone, alpha is dropped), then / 255.  prepare_pair and
    prepare_pair_scaled keep a float image as it is, so the jitter precedes the flip and the resample."""
    if img_u8.dtype != np.uint8:
        raise ValueError(f"apply_photo takes the decoded uint8 image, got {img_u8.dtype}")
    table = np.asarray(table)
    if table.shape != (256,) or table.dtype != np.float32:
        raise ValueError("the tone table is float32 [256]")
    one = img_u8.ndim == 2 or img_u8.shape[2] == 1
    t = gray_to_rgb(table.astype(np.float64)[img_u8])
    if gray and not one:
        w = GRAY_MIX.astype(np.float64)
        y = w[2] * t[..., 2] + (w[1] * t[..., 1] + w[0] * t[..., 0])
        t = np.stack([y, y, y], axis=2)
    return t / 255.0


def normalize_chw(img_hwc: np.ndarray) -> np.ndarray:
    chw = img_hwc.transpose(2, 0, 1).astype(np.float32)
    return (chw - IMAGENET_MEAN[:, None, None]) / IMAGENET_STD[:, None, None]


def prepare_pair(img: np.ndarray, dmap: np.ndarray, downsample: int = 8, flip: bool = False):
    """Full reference transform (model/CrowdDataset.py:38-67): returns (img CHW f32, dmap 1xhxw f32)."""
    img = gray_to_rgb(to_unit_float(img))
    if flip:
        img = img[:, ::-1]
        dmap = dmap[:, ::-1]
    if downsample < 1:
        raise ValueError("downsample must be >= 1")
    rows, cols = img.shape[0] // downsample, img.shape[1] // downsample
    img = resize_linear(np.ascontiguousarray(img), cols * downsample, rows * downsample)
    dm = resize_linear(np.ascontiguousarray(dmap, dtype=np.float32), cols, rows) * (downsample * downsample)
    return normalize_chw(img), dm[None].astype(np.float32)


def area_factor(sh: int, sw: int, rows: int, cols: int) -> np.float32:
    """What a (sh, sw) density window resampled to (rows, cols) cells is multiplied by: source pixels per cell
    (exactly d*d for an unscaled window of (rows*d, cols*d))."""
    return np.float32((sh * sw) / (rows * cols))


def prepare_pair_scaled(img: np.ndarray, dmap: np.ndarray, ch: int, cw: int, downsample: int = 8, flip: bool = False):
    """prepare_pair for a source window of ANY extent (sh, sw) resampled to a (ch, cw) sample (random-scale crops):
    flip within the window, cv2 INTER_LINEAR resize of the image to (cw, ch), normalise; density resized to
    (cw/d, ch/d) x (sh*sw) / cells.  The taps clamp inside the window handed in, so the result is a function of its
    bytes alone; for (sh, sw) == (ch, cw) it is prepare_pair's result bit for bit.  The density stays point-sampled
    (module docstring): a shrunk window (sh > ch) samples every sh/(ch/d)-th pixel pair, coarser than the unscaled
    rule.  Returns (img 3 x ch x cw f32, dmap 1 x ch/d x cw/d f32)."""
    if downsample < 1 or ch <= 0 or cw <= 0 or ch % downsample or cw % downsample:
        raise ValueError(f"sample {ch}x{cw} must be a positive multiple of the downsample {downsample}")
    if tuple(dmap.shape) != tuple(img.shape[:2]):
        raise ValueError(f"density window {tuple(dmap.shape)} differs from its image window {tuple(img.shape[:2])}")
    img = gray_to_rgb(to_unit_float(img))
    if flip:
        img = img[:, ::-1]
        dmap = dmap[:, ::-1]
    sh, sw = img.shape[:2]
    rows, cols = ch // downsample, cw // downsample
    img = resize_linear(np.ascontiguousarray(img), cw, ch)
    dm = resize_linear(np.ascontiguousarray(dmap, dtype=np.float32), cols, rows) * area_factor(sh, sw, rows, cols)
    return normalize_chw(img), dm[None].astype(np.float32)


def _cell_overlaps(ext: int, cells: int, lo: int, hi: int) -> np.ndarray:
    """[cells, hi - lo] float64: the length of source pixel p (lo <= p < hi, window-relative) inside cell i of an axis
    of extent ``ext`` cut into ``cells`` cells: max(0, min((p+1) cells, (i+1) ext) - max(p cells, i ext)) / cells, the
    integers exact."""
    p = np.arange(lo, hi, dtype=np.int64)[None, :]
    i = np.arange(cells, dtype=np.int64)[:, None]
    return np.maximum(0, np.minimum((p + 1) * cells, (i + 1) * ext) - np.maximum(p * cells, i * ext)) / float(cells)


def _head_profile(pos: int, sigma: float, radius: int, off: int, ext: int, cells: int) -> np.ndarray:
    """P[i] = sum_p overlap_i(p) k[off + p - pos] over the window pixels p inside the head's footprint, k the
    normalised, truncated 1-D Gaussian of the head record (a unit delta for sigma <= 0), float64 [cells]."""
    if not sigma > 0:
        radius = 0
    lo, hi = max(0, pos - radius - off), min(ext, pos + radius + 1 - off)
    if lo >= hi:
        return np.zeros(cells)
    if radius == 0:
        k = np.ones(1)
    else:
        t = np.arange(-radius, radius + 1, dtype=np.float64)
        k = np.exp(-(t * t) / (2.0 * sigma * sigma))
        k = k / k.sum()
    return _cell_overlaps(ext, cells, lo, hi) @ k[lo + off - pos + radius:hi + off - pos + radius]


def heads_to_gt64(heads: np.ndarray, h0: int, w0: int, window, ch: int, cw: int, downsample: int = 8,
                  flip: bool = False) -> np.ndarray:
    """heads_to_gt before its float32 rounding: float64 [ch/d, cw/d]."""
    y0, x0, sh, sw = (int(v) for v in window)
    if downsample < 1 or ch <= 0 or cw <= 0 or ch % downsample or cw % downsample:
        raise ValueError(f"sample {ch}x{cw} must be a positive multiple of the downsample {downsample}")
    if sh < 1 or sw < 1 or y0 < 0 or x0 < 0 or y0 + sh > h0 or x0 + sw > w0:
        raise ValueError(f"window {(y0, x0, sh, sw)} is empty or leaves its {h0}x{w0} image")
    rows, cols = ch // downsample, cw // downsample
    out = np.zeros((rows, cols), dtype=np.float64)
    for c, r, sigma, radius in np.asarray(heads, dtype=np.float32).reshape(-1, 4).tolist():
        c, r, radius = int(c), int(r), int(radius)
        if r + radius < y0 or r - radius >= y0 + sh or c + radius < x0 or c - radius >= x0 + sw:
            continue                             # the footprint misses the window: exactly nothing
        out += np.outer(_head_profile(r, sigma, radius, y0, sh, rows), _head_profile(c, sigma, radius, x0, sw, cols))
    return out[:, ::-1] if flip else out


def heads_to_gt(heads: np.ndarray, h0: int, w0: int, window, ch: int, cw: int, downsample: int = 8,
                flip: bool = False) -> np.ndarray:
    """The ground truth of a window rendered from head records (data/density.py:heads_table), no map resampled:
    cell (i, j) of the (ch/d, cw/d) grid is the exact area sum of the density map over the source rectangle it
    covers in window = (y0, x0, sh, sw), every source pixel a unit square of constant density, so the cells sum to
    the window's density mass for any scale, offset and flip, and no area factor is applied.  Per head the sum is
    separable, Py[i] Px[j]; heads are summed in table order in float64.  Returns fp32 [1, ch/d, cw/d]."""
    return heads_to_gt64(heads, h0, w0, window, ch, cw, downsample, flip)[None].astype(np.float32)


def heads_to_gt_padded(heads: np.ndarray, h0: int, w0: int, y0: int, x0: int, ch: int, cw: int, downsample: int = 8,
                       flip: bool = False) -> np.ndarray:
    """heads_to_gt for the UNSCALED crop at (y0, x0): the valid (vh, vw) = crop_window extent of the crop is rendered
    (every cell an exact d x d box sum, flipped within the valid columns) and the cells of the zero padding of an image
    smaller than the crop are 0.  Returns fp32 [1, ch/d, cw/d]."""
    d = downsample
    vh, vw = min(ch, h0 // d * d), min(cw, w0 // d * d)
    out = np.zeros((1, ch // d, cw // d), dtype=np.float32)
    if vh and vw:
        out[:, :vh // d, :vw // d] = heads_to_gt(heads, h0, w0, (y0, x0, vh, vw), vh, vw, d, flip)
    return out


def _overlap_numerators(ext: int, cells: int) -> np.ndarray:
    """int64 [cells, ext]: oy_i(t) = max(0, min((t+1) cells, (i+1) ext) - max(t cells, i ext)), the length of source
    pixel t inside cell i of an axis of extent ``ext`` cut into ``cells`` cells, times ``cells``.  Every row sums to
    ``ext``."""
    t = np.arange(ext, dtype=np.int64)[None, :]
    i = np.arange(cells, dtype=np.int64)[:, None]
    return np.maximum(0, np.minimum((t + 1) * cells, (i + 1) * ext) - np.maximum(t * cells, i * ext))


def roi_weights(mask_u8: np.ndarray, y0: int, x0: int, sh: int, sw: int, rows: int, cols: int,
                flip: bool = False) -> np.ndarray:
    """The per-cell loss weight of a window of an ROI mask (uint8 [H0, W0], 255 inside, 0 outside, a in between the
    fraction a / 255): cell (i, j) of the (rows, cols) grid is the exact area mean of mask / 255 over the source
    rectangle it covers in the window (y0, x0, sh, sw), the rectangle of heads_to_gt, mirrored columns when flipped:
    S = sum_t sum_u oy_i(t) ox_j'(u) a[y0+t][x0+u] in int64, m = float32(float64(S) / float64(255 sh sw)).  All-integer
    up to the one division, so csrc/preprocess.hip roi_weights_kernel gives the same bits; an all-255 window gives
    exactly 1.0.  Returns fp32 [rows, cols]."""
    y0, x0, sh, sw, rows, cols = (int(v) for v in (y0, x0, sh, sw, rows, cols))
    mask_u8 = np.asarray(mask_u8)
    if mask_u8.ndim != 2 or mask_u8.dtype != np.uint8:
        raise ValueError(f"an ROI mask is uint8 [H0, W0], got {mask_u8.dtype} {tuple(mask_u8.shape)}")
    h0, w0 = mask_u8.shape
    if rows < 1 or cols < 1:
        raise ValueError(f"a weight plane needs rows, cols >= 1, got {(rows, cols)}")
    if sh < 1 or sw < 1 or y0 < 0 or x0 < 0 or y0 + sh > h0 or x0 + sw > w0:
        raise ValueError(f"window {(y0, x0, sh, sw)} is empty or leaves its {h0}x{w0} mask")
    a = mask_u8[y0:y0 + sh, x0:x0 + sw].astype(np.int64)
    s = _overlap_numerators(sh, rows) @ a @ _overlap_numerators(sw, cols).T
    m = (s.astype(np.float64) / np.float64(255 * sh * sw)).astype(np.float32)
    return np.ascontiguousarray(m[:, ::-1]) if flip else m


def roi_weights_padded(mask_u8: np.ndarray, y0: int, x0: int, ch: int, cw: int, downsample: int = 8,
                       flip: bool = False) -> np.ndarray:
    """roi_weights for the UNSCALED crop at (y0, x0) of an image that may be smaller than the crop: the valid (vh, vw)
    = crop_window extent is rendered (every cell an exact d x d box, flipped within the valid columns) and the cells of
    the zero padding are 0, so the padding takes no part in the loss.  Returns fp32 [ch/d, cw/d]."""
    d = int(downsample)
    h0, w0 = np.asarray(mask_u8).shape
    vh, vw = min(ch, h0 // d * d), min(cw, w0 // d * d)
    out = np.zeros((ch // d, cw // d), dtype=np.float32)
    if vh and vw:
        out[:vh // d, :vw // d] = roi_weights(mask_u8, y0, x0, vh, vw, vh // d, vw // d, flip)
    return out
