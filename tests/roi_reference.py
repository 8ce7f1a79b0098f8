"""Plain references of the ROI-mask feature (README, "ROI masks and GAME"), written from the definitions with loops:
the per-cell loss weight of a mask window, the count metrics (masked counts and GAME 0..3) and the weighted head's
fp32 staging -- and the cases the CPU and GPU tests share.

Weight plane: cell (i, j) of a window (y0, x0, sh, sw) cut into rows x cols cells covers source rows
[i sh / rows, (i+1) sh / rows) and the columns of j' = cols-1-j when flipped.  With the integer overlap numerators
oy_i(t) = max(0, min((t+1) rows, (i+1) sh) - max(t rows, i sh)) and ox likewise,
S = sum_t sum_u oy_i(t) ox_j'(u) a[y0+t][x0+u] (a Python int) and m = float32(float64(S) / float64(255 sh sw)).
"""
import math
import types

import numpy as np
import torch

import elementwise_reference as R

F64 = torch.float64


# ------------------------------------------------------------------------------------------------------ weight plane
def overlap(i, t, ext, cells):
    return max(0, min((t + 1) * cells, (i + 1) * ext) - max(t * cells, i * ext))


def roi_weights_ref(mask, y0, x0, sh, sw, rows, cols, flip):
    """fp32 [rows, cols], every cell by the double loop of the definition over the WHOLE window (Python integers)."""
    a = np.asarray(mask)
    out = np.zeros((rows, cols), dtype=np.float32)
    oy = [[overlap(i, t, sh, rows) for t in range(sh)] for i in range(rows)]
    ox = [[overlap(j, u, sw, cols) for u in range(sw)] for j in range(cols)]
    us = [[u for u in range(sw) if ox[j][u]] for j in range(cols)]           # the columns a cell touches
    for i in range(rows):
        ts = [t for t in range(sh) if oy[i][t]]
        for j in range(cols):
            jj = cols - 1 - j if flip else j
            s = 0
            for t in ts:
                row = a[y0 + t]
                s += oy[i][t] * sum(ox[jj][u] * int(row[x0 + u]) for u in us[jj])
            out[i, j] = np.float32(np.float64(s) / np.float64(255 * sh * sw))
    return out


def roi_weights_padded_ref(mask, y0, x0, ch, cw, d, flip):
    """The unscaled crop at (y0, x0) of an image that may be smaller than the crop: the valid (vh, vw) cells as exact
    d x d boxes (flipped within the valid columns), 0 in the padding cells."""
    h0, w0 = np.asarray(mask).shape
    vh, vw = min(ch, h0 // d * d), min(cw, w0 // d * d)
    out = np.zeros((ch // d, cw // d), dtype=np.float32)
    if vh and vw:
        out[:vh // d, :vw // d] = roi_weights_ref(mask, y0, x0, vh, vw, vh // d, vw // d, flip)
    return out


def make_mask(h, w, seed, kind):
    """uint8 [h, w]: "binary" random 0 / 255 blobs (5 x 7 blocks, so 8 x 8 cells are inside, outside and cut), "frac" any
    byte, "ones" all 255."""
    g = np.random.default_rng(seed)
    if kind == "ones":
        return np.full((h, w), 255, dtype=np.uint8)
    if kind == "frac":
        return g.integers(0, 256, size=(h, w), dtype=np.uint8)
    blocks = g.integers(0, 2, size=(-(-h // 5), -(-w // 7)), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.kron(blocks, np.ones((5, 7), dtype=np.uint8))[:h, :w])


# (crop ch, cw, scale s): the window is (round(ch / s), round(cw / s)); sh / ch runs from 0.25 to 4
SCALED_WINDOWS = [(16, 24, 1.0), (16, 24, 4.0), (16, 24, 0.25), (40, 56, 0.7), (40, 56, 1.9), (136, 264, 1.0),
                  (136, 264, 3.1), (136, 264, 0.25)]
WHOLE_IMAGE = (37, 53)              # an uncropped sample: rows = 37 // 8, cols = 53 // 8
SMALL_IMAGE = (21, 45)              # an unscaled 32 x 40 crop of it is padded: (vh, vw) = (16, 40)
SMALL_CROP = (32, 40)


def window_of(ch, cw, s):
    return max(1, int(math.floor(ch / s + 0.5))), max(1, int(math.floor(cw / s + 0.5)))


# ----------------------------------------------------------------------------------------------------- count metrics
METRIC_SHAPES = [(1, 1, 1), (2, 5, 7), (3, 8, 8), (1, 13, 17), (2, 96, 128), (1, 135, 240)]


def count_metrics_ref(et, gt, m=None):
    """float64 [n, 6] = (E, G, GAME_0 .. GAME_3) by loops over levels and cells, the cell sums in fp64 (torch sums of
    the exact products).  Returns (out, bound): bound [n, 6] holds what a fixed-order fp64 kernel may differ by, per
    cell sum (N_px + 64) 2^-53 sum |m et| (or |m gt|), for E and G the level-0 cell's own and for GAME_l the sum of
    both bounds over the level's cells."""
    et, gt = et.detach().cpu().to(F64), gt.detach().cpu().to(F64)
    mm = torch.ones_like(et) if m is None else m.detach().cpu().to(F64)
    n, h, w = et.shape
    out = torch.zeros(n, 6, dtype=F64)
    bound = torch.zeros(n, 6, dtype=F64)
    for s in range(n):
        pe, pg = mm[s] * et[s], mm[s] * gt[s]
        for lvl in range(4):
            game = 0.0
            for a in range(1 << lvl):
                r0, r1 = (a * h) >> lvl, ((a + 1) * h) >> lvl
                for b in range(1 << lvl):
                    c0, c1 = (b * w) >> lvl, ((b + 1) * w) >> lvl
                    e, g = pe[r0:r1, c0:c1].sum().item(), pg[r0:r1, c0:c1].sum().item()
                    game += abs(e - g)
                    k = ((r1 - r0) * (c1 - c0) + 64) * 2.0 ** -53
                    be, bg = k * pe[r0:r1, c0:c1].abs().sum().item(), k * pg[r0:r1, c0:c1].abs().sum().item()
                    bound[s, 2 + lvl] += be + bg
                    if lvl == 0:
                        out[s, 0], out[s, 1] = e, g
                        bound[s, 0], bound[s, 1] = be, bg
            out[s, 2 + lvl] = game
    return out, bound


def metric_inputs(n, h, w, seed, exact):
    """(et, gt, m) fp32 [n, h, w].  exact: multiples of 2^-10 with |.| <= 4 (m in [0, 1]), so every product is a
    multiple of 2^-20 and every sum of them exact in fp64 in any order; else random floats."""
    g = torch.Generator().manual_seed(seed)
    if exact:
        et = torch.randint(-4096, 4097, (n, h, w), generator=g).float() / 1024
        gt = torch.randint(0, 4097, (n, h, w), generator=g).float() / 1024
        m = torch.randint(0, 1025, (n, h, w), generator=g).float() / 1024
    else:
        et = torch.randn(n, h, w, generator=g)
        gt = torch.rand(n, h, w, generator=g)
        m = torch.rand(n, h, w, generator=g)
    return et, gt, m


# ------------------------------------------------------------------------------------------------------ weighted head
def head_staged_weighted(et32, y16, w, gt, m, gscale=1.0, lscale=None, pitch=0, wv=0):
    """elementwise_reference.head_staged with the one extra product: in fp32, one rounding per operation in the kernel's
    order, d = et - gt, dm = m d, g = (2 dm) gscale, dy = ((g lscale) w) (y > 0) rounded to y's type (expected bit for
    bit); then the fp64 sums of the staged fp32 values: loss = sum dm d, dw = sum g y, db = sum g, and their magnitude
    sums."""
    P = y16.shape[0]
    f32 = torch.float32
    valid = R.head_valid(P, pitch, wv, y16.device)
    zero = torch.zeros((), dtype=f32, device=y16.device)
    d = torch.where(valid, et32.to(f32) - gt.to(f32), zero)
    dm = m.to(f32) * d
    g = (2.0 * dm) * torch.tensor(gscale, dtype=f32, device=y16.device)
    ls = torch.tensor(1.0 if lscale is None else float(lscale), dtype=f32, device=y16.device)
    o = (g * ls)[:, None] * w.to(f32)[None, :]
    dy = torch.where(y16 > 0, o, zero).to(y16.dtype)
    terms = g.to(F64)[:, None] * y16.to(F64)
    lt = dm.to(F64) * d.to(F64)
    return types.SimpleNamespace(d=d, dm=dm, g=g, dy=dy, valid=valid, loss=lt.sum(), loss_mag=lt.abs().sum(),
                                 dw=terms.sum(0), dw_mag=terms.abs().sum(0), db=g.to(F64).sum(),
                                 db_mag=g.to(F64).abs().sum())


WEIGHTED_HEAD_CASES = [(1, 1), (33, 2), (1000, 15), (1000, 31), (40000, 1024)]


# ------------------------------------------------------------------------------------------------------ small folder
def write_folder(root, sizes, seed=0, heads=True, masks=True, kind="binary"):
    """A small dataset folder root/images/*.jpg + root/ground_truth/*.npy [+ .heads.npy] [+ .roi.npy] of the given
    (h, w) sizes; returns (img_root, gt_root)."""
    import os
    from PIL import Image
    from can_distributed_pytorch_amd.data.density import heads_path, roi_path
    img_root, gt_root = os.path.join(root, "images"), os.path.join(root, "ground_truth")
    os.makedirs(img_root, exist_ok=True)
    os.makedirs(gt_root, exist_ok=True)
    g = np.random.default_rng(seed)
    for k, (h, w) in enumerate(sizes):
        name = f"IMG_{k + 1}"
        Image.fromarray(g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(
            os.path.join(img_root, name + ".jpg"), quality=95)
        npy = os.path.join(gt_root, name + ".npy")
        np.save(npy, (g.random((h, w)) * 0.01).astype(np.float32))
        if heads:
            nh = 6
            rec = np.stack([g.integers(0, w, nh), g.integers(0, h, nh), g.uniform(1.0, 3.0, nh),
                            np.full(nh, 6)], axis=1).astype(np.float32)
            np.save(heads_path(npy), rec)
        if masks:
            np.save(roi_path(npy), make_mask(h, w, seed + 100 + k, kind))
    return img_root, gt_root
