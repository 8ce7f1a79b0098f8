"""Plain fp64 references (numpy, no torch kernels) for the kernels that make the ground truth: csrc/density.hip
(density_knn_kernel, density_splat_kernel, density_fill_kernel) and the synthetic renderer of csrc/preprocess.hip
(synth_gt_kernel, synth_image_kernel), with the error bounds the GPU tests hold the kernels to and the inputs both
test files share.  tests/test_density_reference_cpu.py checks the references against independent code (scipy's KD-tree
and gaussian_filter, torch's bilinear interpolate, the CPU recipe of data/synthetic.py) and shows that the bounds
notice seven wrong variants (built there, from the pieces below); tests/test_gpu_density.py runs the kernels.

u = 2^-24 is the relative error of one fp32 rounding throughout.

Sigma bound (derived): dx and dy are rounded (u each), the two products and their sum put 4 u on the squared distance
v, sqrtf halves that and adds one rounding (3 u), the two adds of the three distances add 2 u, 0.1f is a rounded
constant (u) and the multiply rounds once more (u): 7 u, held as |sigma_gpu - sigma_ref| <= 8 u sigma_ref (SIGMA_ULPS).

Splat bound: a Gaussian factor exp(a), a = -t^2 / (2 sigma^2), is computed as __expf(k t t) with k = -0.5f / (s s): the
roundings of k and of the products are relative errors of the exponent, that is an error (a few u) |a| relative to the
factor, and the hardware exponential adds its own; the normaliser, its reciprocal and the two products add a few u
more.  So a head's contribution is held to C_SPLAT u (1 + |a_y| + |a_x|) of itself, and the fp32 atomic adds of `count`
overlapping footprints, in any order, to count u of the summed value.  C_SPLAT is measured, not derived (the error of
__expf on gfx950 is not documented): see the constant below.

Image bound: A_IMAGE, derived in render_ref's docstring.
"""
import numpy as np

U = 2.0 ** -24
SIGMA_ULPS = 8.0

# The one constant of the splat bound.  Origin: tests/test_gpu_density.py on one MI355X measured the worst
# err / (bound map at C_SPLAT = 1) over every splat case (fixed sigma, kNN, LDS sizes; profiles/r15/density_errors.txt)
# as 2.77 (the single head of sigma 16, R = 64; the fixed-sigma cases reach 0.82, the kNN cases 2.11); 4 x that,
# rounded up to one significant digit.  The ceiling: with this constant the bound stays at or below 1e-4 of the value
# at every in-footprint element of every case (asserted in test_density_reference_cpu.py).
C_SPLAT = 20.0

# 13 roundings counted in render_ref's docstring + 1 for the second-order terms
A_IMAGE = 14.0 * U

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


# ---------------------------------------------------------------------------------------------------------- sigma
def sorted_distances(points_f32):
    """[n, n] fp64: row i holds the distances from head i to every head (itself included: column 0 is 0), ascending,
    computed on the fp32 point values."""
    p = np.asarray(points_f32, dtype=np.float32).astype(np.float64).reshape(-1, 2)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    d.sort(axis=1)
    return d


def sigmas_ref(points_f32, H, W):
    """0.1 * (d1 + d2 + d3) over the neighbours that exist, from brute-force all-pairs distances in fp64 on the fp32
    point values (self included: d0 = 0); one head: (H + W) / 8."""
    n = len(np.asarray(points_f32).reshape(-1, 2))
    if n == 0:
        return np.zeros(0)
    if n == 1:
        return np.array([(H + W) / 8.0])
    return 0.1 * sorted_distances(points_f32)[:, 1:min(4, n)].sum(axis=1)


def radius_f32(sigma_f32, max_r=0):
    """The kernel's radius rule in fp32 arithmetic exactly: int(4 s + 0.5), capped by max_r when max_r > 0."""
    s = np.asarray(sigma_f32, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        rf = np.float32(4) * s + np.float32(0.5)
    r = np.where(rf >= np.float32(2.0e9), 2000000000, rf.astype(np.int64))
    if max_r > 0:
        r = np.minimum(r, max_r)
    return r


def radius_f64(sigma_f64, max_r=0):
    r = (4.0 * np.asarray(sigma_f64, dtype=np.float64) + 0.5).astype(np.int64)
    return np.minimum(r, max_r) if max_r > 0 else r


def radius_margin(sigma_f64):
    """(distance of 4 sigma + 0.5 to the nearest integer) / (4 sigma + 0.5): an fp32 sigma within 8 u of sigma_f64
    cannot give another radius when this is >= 1e-4."""
    rf = 4.0 * np.asarray(sigma_f64, dtype=np.float64) + 0.5
    return np.abs(rf - np.rint(rf)) / rf


def in_image(points_f32, H, W):
    """The heads the splat does not skip: x >= 0, y >= 0, int(x) < W, int(y) < H."""
    p = np.asarray(points_f32, dtype=np.float32).reshape(-1, 2)
    return (p[:, 0] >= 0) & (p[:, 1] >= 0) & (p[:, 0].astype(np.int64) < W) & (p[:, 1].astype(np.int64) < H)


# ---------------------------------------------------------------------------------------------------------- splat
class Splat:
    """value, support (footprints covering each pixel), bound_c (the head term of the bound per unit C_SPLAT) and
    bound_sum (count u value, the order of the atomic adds)."""

    def __init__(self, value, support, bound_c):
        self.value, self.support, self.bound_c = value, support, bound_c
        self.bound_sum = support * U * value

    def bound(self, c=None):
        return (C_SPLAT if c is None else c) * self.bound_c + self.bound_sum


def splat_ref(points_f32, sigma, H, W, max_r=0, radii=None):
    """Sum over the in-image heads of the clipped outer product of two 1-D Gaussians in fp64, each normalised over
    the whole 2R + 1 taps (mass outside the image is dropped after normalising); sigma <= 0 adds 1.0 at
    (int(y), int(x)).  R = radius_f32(sigma) for an fp32 sigma array (the kernel's own sigmas: no ambiguity), the fp64
    rule otherwise; `radii` overrides it."""
    p = np.asarray(points_f32, dtype=np.float32).reshape(-1, 2)
    sig = np.asarray(sigma)
    if sig.ndim == 0:
        sig = np.full(len(p), sig, dtype=sig.dtype)
    if radii is None:
        radii = radius_f32(sig, max_r) if sig.dtype == np.float32 else radius_f64(sig, max_r)
    sig = sig.astype(np.float64)
    value = np.zeros((H, W))
    support = np.zeros((H, W))
    bound_c = np.zeros((H, W))
    inside = in_image(p, H, W)
    for i in range(len(p)):
        px, py = int(p[i, 0]), int(p[i, 1])
        if not inside[i]:
            continue
        s, R = sig[i], int(radii[i])
        if s <= 0:
            value[py, px] += 1.0
            support[py, px] += 1
            continue
        y0, y1, x0, x1 = max(0, py - R), min(H - 1, py + R), max(0, px - R), min(W - 1, px + R)
        ay = -((np.arange(y0, y1 + 1) - py) ** 2.0) / (2.0 * s * s)
        ax = -((np.arange(x0, x1 + 1) - px) ** 2.0) / (2.0 * s * s)
        norm = np.exp(-(np.arange(-R, R + 1) ** 2.0) / (2.0 * s * s)).sum()
        ky, kx = np.exp(ay) / norm, np.exp(ax) / norm
        contrib = np.outer(ky, kx)
        value[y0:y1 + 1, x0:x1 + 1] += contrib
        support[y0:y1 + 1, x0:x1 + 1] += 1
        bound_c[y0:y1 + 1, x0:x1 + 1] += U * (1.0 + np.abs(ay)[:, None] + np.abs(ax)[None, :]) * contrib
    return Splat(value, support, bound_c)


# --------------------------------------------------------------------------------------------------------- render
def upsample16(noise):
    """[n, 3, Hn, Wn] -> [n, 3, 16 Hn, 16 Wn]: half-pixel bilinear with clamped taps, the rule of
    data/transforms._axis_weights, in fp64."""
    from can_distributed_pytorch_amd.data.transforms import _axis_weights
    a = np.asarray(noise, dtype=np.float64)
    Hn, Wn = a.shape[-2:]
    y0, y1, fy = _axis_weights(Hn, 16 * Hn)
    x0, x1, fx = _axis_weights(Wn, 16 * Wn)
    rows = a[:, :, y0] * (1.0 - fy)[:, None] + a[:, :, y1] * fy[:, None]
    return rows[..., x0] * (1.0 - fx) + rows[..., x1] * fx


def half_ulp16(x, dtype_name):
    """Half the spacing of bf16 (8 significant bits) or fp16 (11, subnormals below 2^-14) numbers at |x|."""
    _, e = np.frexp(np.abs(x))                       # |x| in [2^(e-1), 2^e)
    e = e.astype(np.float64) - 1.0
    if dtype_name == "bf16":
        return 0.5 * np.exp2(np.maximum(e, -126.0) - 7.0)
    return 0.5 * np.exp2(np.maximum(e, -14.0) - 10.0)


class Render:
    """gt [n, H/8, W/8] and its bound, dmax [n] (fp32, exact), img [n, 3, H, W] (fp64, ImageNet-normalised)."""

    def __init__(self, gt, gt_bound, dmax, img):
        self.gt, self.gt_bound, self.dmax, self.img = gt, gt_bound, dmax, img

    def img_bound(self, dtype_name, extra=0.0):
        """Half a 16-bit ulp of the fp64 value (taken at the far end of the fp32 allowance, so a value the allowance
        carries over a power of two is covered) + A_IMAGE / std_c + extra (an error of the input, already in units
        of the normalised image)."""
        allow = A_IMAGE / np.array(IMAGENET_STD).reshape(1, 3, 1, 1) + extra
        return half_ulp16(np.abs(self.img) + allow, dtype_name) + allow


def pool8(dens):
    """(8x8 block sums [n, H/8, W/8] in fp64, their bound 2 * 64 u sum|v|)."""
    d = np.asarray(dens).astype(np.float64)
    n, H, W = d.shape
    blocks = d.reshape(n, H // 8, 8, W // 8, 8)
    return blocks.sum(axis=(2, 4)), 2 * 64 * U * np.abs(blocks).sum(axis=(2, 4))


def normalise(v):
    """[n, 3, H, W] in [0, 1] -> (v - mean_c) / std_c."""
    return (v - np.array(IMAGENET_MEAN).reshape(1, 3, 1, 1)) / np.array(IMAGENET_STD).reshape(1, 3, 1, 1)


def blend(up, dens, dmax):
    """clip(0.7 up + 0.3 dens / (dmax + float32(1e-6)), 0, 1): up [n, 3, H, W], dens [n, H, W], dmax [n]."""
    eps = np.float64(np.float32(1e-6))
    blob = 0.3 * np.asarray(dens).astype(np.float64) / (np.asarray(dmax).astype(np.float64) + eps)[:, None, None]
    return np.clip(0.7 * up + blob[:, None], 0.0, 1.0)


def render_ref(dens, noise_f32):
    """The synthetic renderer in fp64.  dens [n, H, W] (fp32 values; fp64 accepted for the end-to-end reference),
    noise [n, 3, H/16, W/16].  gt = 8x8 block sums, dmax = per-image max, image =
    clip(0.7 up + 0.3 dens / (dmax + float32(1e-6)), 0, 1), then (v - mean_c) / std_c.

    Bounds.  gt: 2 * 64 u sum|v| per cell (64 sequential fp32 adds).  dmax: exact.  Image: half a 16-bit ulp of the
    value + A_IMAGE / std_c, A_IMAGE counted on values in [0, 1] (every rounding at most u; fused multiply-adds only
    remove roundings).  H = 16 Hn, so the tap weights ((o + 0.5) / 16 - 0.5 and its fraction) are exact in fp32.
      top = a + (b - a) fx : 3 roundings, 3 u; bot the same
      top + (bot - top) fy : (1 - fy) e_top + fy e_bot <= 3 u, + 3 roundings       -> up within 6 u
      0.7f up              : 0.7 * 6 u + the constant's 0.7 u + 1 rounding          -> 5.9 u
      0.3f d inv           : inv = 1 / (dmax + 1e-6f) 2 roundings, 0.3f one, two products: 5 u of <= 0.3 -> 1.5 u
      their sum            : 1 rounding                                             -> 8.4 u before the clip
      v - m[c]             : the constant's 0.5 u + 1 rounding                      -> 9.9 u
      (.) * (1.f / std_f)  : std_f, the division and the product: 3 u |v - m| <= 3 u -> 12.9 u / std_c
    13 u, and 1 u more for the second-order terms: A_IMAGE = 14 u."""
    n = np.asarray(dens).shape[0]
    nz = np.asarray(noise_f32, dtype=np.float32).astype(np.float64)
    gt, gt_bound = pool8(dens)
    dmax = np.asarray(dens).reshape(n, -1).max(axis=1)
    return Render(gt, gt_bound, dmax, normalise(blend(upsample16(nz), dens, dmax)))


def words_to_f64(x4_words_i16, dtype_name):
    """The 16-bit words of an NHWC4 tensor (int16 numpy [..., 4]) -> (img [n, 3, H, W] fp64, channel-3 words)."""
    w = np.ascontiguousarray(x4_words_i16).view(np.uint16)
    if dtype_name == "bf16":
        f = (w.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    else:
        f = w.view(np.float16).astype(np.float64)
    return np.moveaxis(f[..., :3], -1, 1), w[..., 3]


# ---------------------------------------------------------------------------------------------------- shared inputs
KNN_H, KNN_W = 48, 80
# n -> seed (100 + n): with knn_points' draw no in-image head of any of them has a radius margin below 1e-4
# (test_density_reference_cpu.py asserts it; the least is 1.13e-4 at n = 256)
KNN_SEEDS = {2: 102, 3: 103, 4: 104, 5: 105, 255: 355, 256: 356, 257: 357, 513: 613}


def knn_points(n, seed=None):
    """n points uniform over the image grown by 4 px on every side (about a fifth outside), fp32 [[x, y], ...]."""
    rng = np.random.default_rng(KNN_SEEDS[n] if seed is None else seed)
    x = rng.random(n) * (KNN_W + 8) - 4
    y = rng.random(n) * (KNN_H + 8) - 4
    return np.stack([x, y], 1).astype(np.float32)


def knn_duplicate_points():
    """12 points, two of them identical and in the image (d1 = 0 for both)."""
    p = knn_points(12, seed=7)
    p[0] = (31.25, 20.5)
    p[5] = p[0]
    return p


def knn_coincident_points():
    """4 points at one place: every sigma is 0, the map is 4.0 at (7, 10)."""
    return np.tile(np.array([[10.5, 7.25]], dtype=np.float32), (4, 1))


def knn_cases():
    """name -> points, every kNN case of the GPU file (n = 1 apart)."""
    cases = {f"n={n}": knn_points(n) for n in KNN_SEEDS}
    cases["duplicate"] = knn_duplicate_points()
    cases["coincident"] = knn_coincident_points()
    return cases


def edge_heads(H, W):
    """The two corners, a head in the last column, three heads outside (left of 0 by half a pixel, at x = W, below the
    image): [[x, y], ...]."""
    return np.array([[0, 0], [W - 1, H - 1], [W - 0.25, 0.5], [-0.5, H / 2], [W, H / 3], [W / 2, H + 3]],
                    dtype=np.float32)


def overlap_heads(H=48, W=80):
    """40 heads whose sigma-4 footprints (R = 16) overlap and lie inside the 48 x 80 image."""
    rng = np.random.default_rng(40)
    return np.stack([20 + rng.random(40) * 40, 17 + rng.random(40) * 14], 1).astype(np.float32)


INTERIOR = np.array([[40.3, 24.6]], dtype=np.float32)

# name -> (H, W, sigma, max_r, points, the map sums to the number of heads)
SPLAT_CASES = {
    "s0.124_edges": (48, 80, 0.124, 0, edge_heads(48, 80), False),
    "s0.124_interior": (48, 80, 0.124, 0, INTERIOR, True),
    "s0.3_edges": (48, 80, 0.3, 0, edge_heads(48, 80), False),
    "s0.3_interior": (48, 80, 0.3, 0, INTERIOR, True),
    "s4_edges": (48, 80, 4.0, 0, edge_heads(48, 80), False),
    "s4_interior": (48, 80, 4.0, 0, INTERIOR, True),
    "s70_edges": (48, 80, 70.0, 0, np.concatenate([edge_heads(48, 80), INTERIOR]), False),
    "s300_64x96": (64, 96, 300.0, 0, np.concatenate([edge_heads(64, 96), INTERIOR]), False),
    "s4_maxr5_edges": (48, 80, 4.0, 5, edge_heads(48, 80), False),
    "s4_maxr5_interior": (48, 80, 4.0, 5, INTERIOR, True),
    "s4_overlap40": (48, 80, 4.0, 0, overlap_heads(), True),
}

# the dynamic-LDS sizes: (H + W) * 4 bytes of weight tables
LDS_CASES = {
    "lds_65664": (16, 16400, 4.0, 0, np.array([[16399.5, 8.0], [0, 0], [8000.2, 3.3], [16392.0, 15.9]],
                                              dtype=np.float32), False),
    "lds_153600": (8, 38392, 4.0, 0, np.array([[38391.9, 7.5], [100.0, 4.0], [20000.5, 0.0]], dtype=np.float32),
                   False),
}
LDS_REFUSED = (16, 38400)

# (n, H, W): the render shapes; the last one is bf16 only
RENDER_SHAPES = [(1, 16, 16), (2, 32, 48), (3, 48, 80)]
RENDER_LARGE = (1, 2048, 2064)


def render_inputs(n, H, W, seed, variant=None):
    """Hand-made non-negative dens [n, H, W] and noise [n, 3, H/16, W/16], fp32.  variant "scaled": image 1 times 100;
    "zero0": image 0 all zero."""
    rng = np.random.default_rng(seed)
    dens = (rng.random((n, H, W)) ** 4 * 0.05).astype(np.float32)
    noise = rng.random((n, 3, H // 16, W // 16)).astype(np.float32)
    if variant == "scaled":
        dens[1] *= np.float32(100)
    if variant == "zero0":
        dens[0] = 0
    return dens, noise


# (h, w, seed, heads): the shapes at which the CPU recipe and the generator are compared with the references
SYNTH_CASES = [(128, 192, 5, (50, 60)), (16, 16, 1, (3, 3)), (64, 96, 2, (100, 130))]


def draw_synthetic(seed, h, w, heads):
    """The points [n, 2] and the noise grid [3, h/16, w/16] of one image, drawn from the seed in the order of
    data/synthetic.py (head count, points, noise): numpy fp32."""
    import torch
    from can_distributed_pytorch_amd.data.synthetic import synthetic_points
    gen = torch.Generator().manual_seed(int(seed))
    n = int(torch.randint(heads[0], heads[1] + 1, (1,), generator=gen))
    pts = synthetic_points(n, h, w, gen)
    noise = torch.rand(3, h // 16, w // 16, generator=gen)
    return pts.numpy().astype(np.float32), noise.numpy().astype(np.float32)


def synthetic_ref(seed, h, w, heads):
    """(Render of one image, the splat's value and bound maps): render_ref(splat_ref(points, 4.0), noise)."""
    pts, noise = draw_synthetic(seed, h, w, heads)
    sp = splat_ref(pts, np.float32(4.0), h, w)
    return render_ref(sp.value[None], noise[None]), sp


def worst_ratio(err, bound):
    """max err / bound over the elements (0 / 0 counts as 0, x / 0 as inf)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0

