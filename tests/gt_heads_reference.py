"""Plain fp64 oracle for ground truth rendered from head records (data/transforms.py:heads_to_gt on the CPU,
csrc/density.hip:gt_from_heads_kernel on the GPU), written from the definition and sharing no code with either:

  D[y][x] = sum_heads k[y - r] k[x - c] on the H0 x W0 image, k the normalised 1-D Gaussian truncated at the STORED
  radius R, sigma the stored float32 value (sigma <= 0: a unit delta);
  gt = Oy D Ox^T, Oy [rows x H0] and Ox [cols x W0] the rational overlaps of every source pixel (a unit square) with
  the cells of the window, columns mirrored when flipped.

``gt_terms`` is the same sum taken head by head, with what the GPU bound needs: per cell and head the fp64
contribution c_h, the largest Gaussian exponents A_y, A_x among the terms of its two profile entries and their numbers
n_y, n_x, and n_h, the heads that reach the cell.  The bound (u = 2^-24, the project's error model for __expf terms,
20 u (1 + |a|), README round 15):

  u [ sum_h c_h (20 (1 + A_y + A_x) + n_y + n_x + 2) + (n_h - 1) sum_h c_h ]
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
C_EXP = 20.0


def kernel1d(sigma, radius):
    """k[t], t = -R..R, fp64, for the float32 sigma stored in a record; a delta for sigma <= 0."""
    sigma = float(np.float32(sigma))
    if not sigma > 0:
        return np.ones(1), 0
    radius = int(radius)
    t = np.arange(-radius, radius + 1, dtype=np.float64)
    k = np.exp(-(t ** 2) / (2.0 * sigma ** 2))
    return k / k.sum(), radius


def density_from_heads(heads, H0, W0):
    """D [H0, W0] fp64 straight from the definition (mass outside the image is lost after normalising)."""
    D = np.zeros((H0, W0))
    for c, r, s, R in np.asarray(heads, dtype=np.float64).reshape(-1, 4):
        k, R = kernel1d(s, R)
        c, r = int(c), int(r)
        for y in range(max(0, r - R), min(H0, r + R + 1)):
            x0, x1 = max(0, c - R), min(W0, c + R + 1)
            D[y, x0:x1] += k[y - r + R] * k[x0 - c + R:x1 - c + R]
    return D


def overlap_matrix(off, ext, cells, size):
    """[cells, size] fp64: O[i][off + t] = max(0, min((t+1) cells, (i+1) ext) - max(t cells, i ext)) / cells for
    0 <= t < ext, exact rationals (python ints over cells), 0 outside the window."""
    O = np.zeros((cells, size))
    for i in range(cells):
        for t in range(ext):
            num = min((t + 1) * cells, (i + 1) * ext) - max(t * cells, i * ext)
            if num > 0:
                O[i, off + t] = float(Fraction(num, cells))
    return O


def gt_oracle(heads, H0, W0, window, rows, cols, flip, D=None):
    """Oy D Ox^T [rows, cols] fp64, columns mirrored when flipped."""
    y0, x0, sh, sw = window
    D = density_from_heads(heads, H0, W0) if D is None else D
    g = overlap_matrix(y0, sh, rows, H0) @ D @ overlap_matrix(x0, sw, cols, W0).T
    return g[:, ::-1] if flip else g


def _axis_terms(pos, sigma, radius, O):
    """Per cell of one axis and one head: (profile entry, largest exponent among its terms, number of terms)."""
    k, R = kernel1d(sigma, radius)
    size = O.shape[1]
    kv, a = np.zeros(size), np.zeros(size)
    inside = np.zeros(size, dtype=bool)
    lo, hi = max(0, pos - R), min(size, pos + R + 1)
    if lo < hi:
        kv[lo:hi] = k[lo - pos + R:hi - pos + R]
        s = float(np.float32(sigma))
        if s > 0 and R > 0:
            a[lo:hi] = (np.arange(lo, hi) - pos) ** 2.0 / (2.0 * s * s)
        inside[lo:hi] = True
    used = (O > 0) & inside[None, :]
    return O @ kv, np.where(used, a[None, :], 0.0).max(axis=1), used.sum(axis=1)


class Terms:
    """value [rows, cols] (heads summed in table order), bound, reached (heads whose footprint reaches the cell)."""

    def __init__(self, value, bound, reached):
        self.value, self.bound, self.reached = value, bound, reached


def gt_terms(heads, H0, W0, window, rows, cols, flip):
    y0, x0, sh, sw = window
    Oy, Ox = overlap_matrix(y0, sh, rows, H0), overlap_matrix(x0, sw, cols, W0)
    value, head_term, reached = np.zeros((rows, cols)), np.zeros((rows, cols)), np.zeros((rows, cols))
    for c, r, s, R in np.asarray(heads, dtype=np.float64).reshape(-1, 4):
        py, ay, ny = _axis_terms(int(r), s, R, Oy)
        px, ax, nx = _axis_terms(int(c), s, R, Ox)
        ch = np.outer(py, px)
        value += ch
        head_term += ch * (C_EXP * (1.0 + ay[:, None] + ax[None, :]) + ny[:, None] + nx[None, :] + 2.0)
        reached += np.outer(ny > 0, nx > 0)
    bound = U * (head_term + np.maximum(reached - 1.0, 0.0) * value)
    if flip:
        value, bound, reached = value[:, ::-1], bound[:, ::-1], reached[:, ::-1]
    return Terms(value, bound, reached)


def padded_terms(heads, H0, W0, y0, x0, ch, cw, d, flip):
    """gt_terms of the unscaled crop at (y0, x0): the valid extent rendered, the padding cells 0 with bound 0."""
    vh, vw = min(ch, H0 // d * d), min(cw, W0 // d * d)
    value, bound, reached = (np.zeros((ch // d, cw // d)) for _ in range(3))
    if vh and vw:
        t = gt_terms(heads, H0, W0, (y0, x0, vh, vw), vh // d, vw // d, flip)
        value[:vh // d, :vw // d], bound[:vh // d, :vw // d], reached[:vh // d, :vw // d] = t.value, t.bound, t.reached
    return Terms(value, bound, reached)


def box_sums(D, y0, x0, vh, vw, d, flip):
    """The d x d box sums of D's window, flipped within the window."""
    g = D[y0:y0 + vh, x0:x0 + vw].reshape(vh // d, d, vw // d, d).sum(axis=(1, 3))
    return g[:, ::-1] if flip else g


def worst_ratio(err, bound):
    """max err / bound over the elements (0 / 0 counts as 0, x / 0 as inf)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------------ shared inputs
def record(c, r, sigma):
    """One head record with the radius rule of heads_table."""
    return (c, r, sigma, int(4.0 * sigma + 0.5) if sigma > 0 else 0)


def mixed_heads(H0, W0, n, seed):
    """n records at random pixels, sigmas cycling through 0.6, 2, 4 and (every 50th) a delta."""
    rng = np.random.default_rng(seed)
    sig = [0.6, 2.0, 4.0]
    rows = [record(int(rng.integers(0, W0)), int(rng.integers(0, H0)), 0.0 if i % 50 == 49 else sig[i % 3])
            for i in range(n)]
    return np.asarray(rows, dtype=np.float32).reshape(-1, 4)


def edge_heads(H0, W0, window):
    """Heads on the window's first and last row and column, outside it within reach (footprints cut by the window), in
    the image's corners (cut by the image), a delta on the window's last pixel and one of sigma 30 (R = 120, larger
    than any test image)."""
    y0, x0, sh, sw = window
    y1, x1 = y0 + sh - 1, x0 + sw - 1
    rows = [record(x0, y0, 2.0), record(x1, y1, 2.0), record(x0, y1, 0.6), record(x1, y0, 4.0),
            record(max(0, x0 - 3), (y0 + y1) // 2, 2.0), record(min(W0 - 1, x1 + 5), y0, 4.0),
            record(0, 0, 4.0), record(W0 - 1, H0 - 1, 2.0), record(x1, y1, 0.0), record((x0 + x1) // 2, (y0 + y1) // 2, 30.0)]
    return np.asarray(rows, dtype=np.float32).reshape(-1, 4)
