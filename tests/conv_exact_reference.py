"""Exact references of the implicit-GEMM conv kernels (csrc/conv_igemm.hip, csrc/conv_wgrad.hip and its .inc files)
for operands that are small integers times a power of two.

With such operands every product is an integer multiple of one unit 2^-s, and so is every partial sum in any order.  As
long as the sum of the absolute values of the terms of an output, in units, stays below 2^24 (``exactness_bound``),
every partial sum is exactly representable in fp32 -- whatever the MFMA grouping, the split-K part order, the slab
reduction order or the wave layout.  The kernel's fp32 accumulator is then the mathematical result, a 16-bit output is
its single round-to-nearest-even (``to16``) and an fp32 output is the result itself: the tests compare with
``torch.equal`` and there is no tolerance to choose.

The references are fp64, written as shifted sums of matmuls (one per tap, explicit zero padding) in plain torch on the
device of their inputs; they call no convolution or pooling library.  Activations are NHWC, weights have the PyTorch
layout [Co][Ci][kh][kw].  The max-pool code layout and its tie rule are taken from tests/elementwise_reference.py
(``maxpool_ref`` / ``unpack_codes``), not re-derived here.  tests/test_conv_exact_reference_cpu.py checks all of this
against F.conv2d and autograd in float64 on the CPU.
"""
import torch

from elementwise_reference import maxpool_ref, unpack_codes

F64 = torch.float64
LIMIT = 2.0 ** 24                    # integers of magnitude <= 2^24 are exact in fp32
MANT = {torch.bfloat16: 8, torch.float16: 11}      # significand bits (hidden bit included)

# Operand ranges (lo, hi, shift: integers in [lo, hi] times 2^-shift) of the GPU test families.
X_ACT = (-12, 12, 0)                 # activations / incoming gradients of forward and data-gradient convs
W_FWD = (-32, 32, 6)                 # weights
B_FWD = (-16, 16, 2)                 # bias
X_WG = (-3, 3, 0)                    # both operands of a weight gradient (M up to 262144)
X_FIRST = (-100, 100, 0)             # first-layer images (K = 27: with |x| <= 12 fp16 would have next to nothing to round)
POOL_MAP = (-3, 3, 0)                # pool inputs behind EPI_POOLBWD codes: few distinct values, so ties abound
W_BP = (-128, 128, 8)                # weights of the bias-partial families (with sparse_density: few, large terms)


def sparse_density(K, M):
    """Share of non-zero elements of both operands (X_ACT activations, W_BP weights) of a bias-partial case with K
    terms per output and M pixels per channel.  A partial's bound is the sum over the pixels of the per-pixel bound
    K p E|x| E|w| (p = density^2, E|x| = 6.24, E|w| = 64.5 units: 402 per term); p is set so that M of them reach 60 %
    of 2^24, the rest being room for the spread between channels.  Few large terms rather than many small ones: the
    values keep a standard deviation of about 535 sqrt(K p) units, enough of them beyond 2^8 (bf16) and 2^11 (fp16)
    units to need rounding."""
    p = min(1.0, 0.6 * LIMIT / (M * K * 402.0))
    return p ** 0.5


# ----------------------------------------------------------------------------------------------------------- operands
def int_operand(shape, rng, dtype, seed, device="cpu", density=1.0):
    """Seeded integers in [lo, hi] times 2^-shift (``rng`` = (lo, hi, shift)); with density < 1 that share of the
    elements is kept and the rest set to 0.  Returns (tensor of ``dtype``, its fp64 copy), both on ``device``; asserts
    that the two are equal, so the operand really is representable.  dtype may be torch.float32 (bias, dw0)."""
    lo, hi, shift = rng
    g = torch.Generator(device=device).manual_seed(seed)           # drawn on the device: the large maps stay there
    v = torch.randint(lo, hi + 1, tuple(shape), generator=g, device=device).to(F64) * 2.0 ** -shift
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=g, device=device) < density)
    t = v.to(dtype)
    assert torch.equal(t.to(F64), v), f"operand range {rng} is not representable in {dtype}"
    return t, v


def relu_operand(shape, rng, dtype, seed, device="cpu"):
    """A post-ReLU map of ``int_operand`` values (a pool input)."""
    t, v = int_operand(shape, rng, dtype, seed, device)
    return torch.relu(t), torch.relu(v)


# --------------------------------------------------------------------------------------------------------- references
def _taps(ksize, dil):
    """(kh, kw, dy, dx): tap (kh, kw) of a 'same'-padded conv reads the input at (h + dy, w + dx)."""
    r = ksize // 2
    return [(kh, kw, (kh - r) * dil, (kw - r) * dil) for kh in range(ksize) for kw in range(ksize)]


def shifted(x, dy, dx):
    """s[n, h, w] = x[n, h + dy, w + dx] where that is inside the map, 0 elsewhere (the explicit zero padding)."""
    n, h, w, c = x.shape
    out = torch.zeros_like(x)
    h0, h1 = max(0, -dy), min(h, h - dy)
    w0, w1 = max(0, -dx), min(w, w - dx)
    if h0 < h1 and w0 < w1:
        out[:, h0:h1, w0:w1] = x[:, h0 + dy:h1 + dy, w0 + dx:w1 + dx]
    return out


def conv_ref(x, w, dil=1):
    """y[n, h, w, co] = sum_{kh, kw, ci} x[n, h + dy, w + dx, ci] w[co, ci, kh, kw]  (fp64)."""
    n, h, wd, ci = x.shape
    co, _, k, _ = w.shape
    y = torch.zeros(n * h * wd, co, dtype=F64, device=x.device)
    for kh, kw, dy, dx in _taps(k, dil):
        y += shifted(x, dy, dx).reshape(-1, ci) @ w[:, :, kh, kw].t()
    return y.reshape(n, h, wd, co)


def conv_fwd_ref(x, w, b, dil=1, epi="bias_relu"):
    """The forward epilogues: 'bias_relu' relu(conv + b), 'bias' conv + b, 'none' conv."""
    y = conv_ref(x, w, dil)
    if epi == "none":
        return y
    y = y + b
    return torch.relu(y) if epi == "bias_relu" else y


def dgrad_ref(dy, w, dil=1):
    """dx[n, h, w, ci] = sum_{kh, kw, co} dy[n, h - dy_, w - dx_, co] w[co, ci, kh, kw]: the data gradient of the
    layer whose weight is w [Co][Ci][kh][kw]."""
    n, h, wd, co = dy.shape
    _, ci, k, _ = w.shape
    out = torch.zeros(n * h * wd, ci, dtype=F64, device=dy.device)
    for kh, kw, sy, sx in _taps(k, dil):
        out += shifted(dy, -sy, -sx).reshape(-1, co) @ w[:, :, kh, kw]
    return out.reshape(n, h, wd, ci)


def dgrad_mask_ref(dy, w, mask, dil=1):
    """EPI_MASK: the data gradient where mask > 0, 0 elsewhere."""
    d = dgrad_ref(dy, w, dil)
    return torch.where(mask > 0, d, torch.zeros((), dtype=F64, device=d.device))


def poolbwd_ref(d, codes):
    """EPI_POOLBWD: d [n, h, w, c] is the gradient of a 2x2 max-pool's output, codes its max-pool codes; the gradient
    of the pool input [n, 2h, 2w, c] gets d at the one window position whose code bit is set (bit p = position
    (p // 2, p % 2)), 0 elsewhere -- none where the code is 0 (an all-zero window: the ReLU mask)."""
    n, h, w, c = d.shape
    nib = unpack_codes(codes)
    out = torch.zeros(n, 2 * h, 2 * w, c, dtype=d.dtype, device=d.device)
    for p in range(4):
        out[:, p // 2::2, p % 2::2] = d * ((nib >> p) & 1).to(d.dtype)
    return out


def wgrad_ref(dy, x, ksize, dil=1):
    """(dw [Co][Ci][kh][kw], db [Co]): dw = sum_m dy[m, co] x[m + tap, ci], db = sum_m dy[m, co]  (fp64)."""
    n, h, w, ci = x.shape
    co = dy.shape[-1]
    d2 = dy.reshape(-1, co).t().contiguous()
    dw = torch.zeros(co, ci, ksize, ksize, dtype=F64, device=x.device)
    for kh, kw, sy, sx in _taps(ksize, dil):
        dw[:, :, kh, kw] = d2 @ shifted(x, sy, sx).reshape(-1, ci)
    return dw, d2.sum(1)


def wgrad_update_ref(g, g0=None, beta=0.0, scale=1.0, dscale=1.0):
    """What conv_wgrad writes: scale * dscale * g (+ beta * g0)."""
    out = (scale * dscale) * g
    return out + beta * g0 if beta != 0.0 else out


def first3(x4):
    """NHWC4 first-layer input -> its three image channels."""
    return x4[..., :3].contiguous()


def conv_first_ref(x4, w, b, epi="bias_relu"):
    """First layer: x4 [n, h, w, 4] (channel 3 is padding), w [Co][3][3][3]."""
    return conv_fwd_ref(first3(x4), w, b, 1, epi)


def wgrad_first_ref(dy, x4):
    return wgrad_ref(dy, first3(x4), 3, 1)


def pool_fwd_ref(x, w, b, dtype, dil=1):
    """The fused conv + bias + ReLU + 2x2 max-pool: (full map, pooled map, codes), the first two in ``dtype``.  The pool
    runs on the rounded outputs; codes and ties as elementwise_reference.maxpool_ref."""
    full = to16(conv_fwd_ref(x, w, b, dil), dtype)
    pooled, codes, _ = maxpool_ref(full)
    return full, pooled, codes


# ------------------------------------------------------------------------------------------------ bound, rounding, stats
def exactness_bound(ref, operands, shift):
    """max over the outputs of ``ref`` applied to the operands' absolute values, in units of 2^-shift (shift = the sum
    of the shifts of the multiplied operands, at least that of any added one): the sum of the absolute values of an
    output's terms, which bounds every partial sum of them in every order.  Below 2^24, fp32 sums them exactly."""
    out = ref(*[o.abs() for o in operands])
    if isinstance(out, (tuple, list)):
        return max(float(o.max()) for o in out) * 2.0 ** shift
    return float(out.max()) * 2.0 ** shift


def bias_partial_bound(ref, operands, shift):
    """The bound of a bias partial: the per-channel sum over every pixel of the batch of the per-pixel bound (any
    subset of pixels a partial row covers sums to no more)."""
    out = ref(*[o.abs() for o in operands])
    return float(out.reshape(-1, out.shape[-1]).sum(0).max()) * 2.0 ** shift


def to32(ref64):
    """fp64 -> fp32, asserted exact (it is whenever the bound holds)."""
    f = ref64.to(torch.float32)
    assert torch.equal(f.to(F64), ref64), "reference is not exactly representable in fp32"
    return f


def to16(ref64, dtype):
    """The one rounding: fp64 -> fp32 (exact, asserted) -> dtype, round to nearest even."""
    out = to32(ref64).to(dtype)
    assert bool(torch.isfinite(out).all()), f"reference overflows {dtype}"
    return out


def rounding_stats(ref64, dtype):
    """(share of the non-zero reference outputs that are not representable in ``dtype``, number that are exact ties:
    halfway between two neighbouring values of ``dtype``).  Normal range only (asserted)."""
    v = ref64.reshape(-1)
    v = v[v != 0]
    if v.numel() == 0:
        return 0.0, 0
    assert float(v.abs().min()) >= 2.0 ** -14, "subnormal outputs: the spacing below is for normal numbers"
    r = v.to(torch.float32).to(dtype).to(F64)
    err = (v - r).abs()
    _, e = torch.frexp(v)                                # |v| = m 2^e, m in [0.5, 1)
    spacing = torch.ldexp(torch.ones_like(v), e - MANT[dtype])
    return float((err != 0).sum()) / v.numel(), int((err * 2 == spacing).sum())
