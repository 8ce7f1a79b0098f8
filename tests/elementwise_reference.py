"""Plain references of the memory-bound kernels of csrc/elementwise.hip: the training head (head_fwd, head_train,
head_reduce), the 2x2 max-pool and its two backwards, the split-bf16 operand builders (split_x3), the device-side loss
scaler (scale_update) -- and the error bounds the GPU tests hold the kernels to.

Every reference is fp64, or exact integer / bit logic, written from the definitions (model/CANNet.py: output_layer and
MSELoss(sum), nn.MaxPool2d(2, 2)) and the kernels' header comments, in plain torch on the device of its inputs.  Nothing
here calls ATen's pooling or convolution; tests/test_elementwise_reference_cpu.py compares these references with ATen
on the CPU and shows that the bounds notice a dropped block partial, a skipped reduce tail and a one-ulp error.

Head layouts: y16 [P, 64] 16-bit post-ReLU activations, w [64], b a scalar, gt [P].  A width-padded map has rows of
``pitch`` pixels of which the first ``wv`` are valid (pitch <= wv: no padding).
"""
import math
import struct
import types

import torch

F64 = torch.float64
U24 = 2.0 ** -24                    # unit roundoff of fp32

# (P, nblk) of the head tests: one block and fewer pixels than a block holds; 14..16 and 29..31 blocks around the
# 15-group reduce's unrolled body and its tail; 46 blocks (more than the pixels fill: empty blocks write zeros);
# 40000 and 70001 pixels on 1024 blocks: the second and third grid sweep of head_train, 70001 the second of head_fwd.
HEAD_CASES = [(1, 1), (7, 1), (33, 2), (1000, 14), (1000, 15), (1000, 16), (1000, 29), (1000, 30), (1000, 31),
              (1000, 46), (40000, 1024), (70001, 1024)]
# (gscale, lscale, beta): both gradient scales with and without a loss scale, beta 0 / 0.5 / 1
HEAD_CONFIGS = [(1.0, None, 0.0), (0.25, 1024.0, 0.5), (1.0, 1024.0, 1.0), (0.25, None, 0.0)]
# (rows, pitch, wv) of the width-padded head tests; the last has no padding columns
HEAD_PADDED = [(10, 24, 17), (6, 8, 1), (5, 16, 16)]
REDUCE_GROUPS = 15                  # head_reduce_kernel's G
HEAD_ET_DEPTH = 12                  # 8 fma, 3 butterfly adds, 1 bias add


# ------------------------------------------------------------------------------------------------------------- head
def head_valid(P, pitch, wv, device=None):
    """[P] bool: pixel p is a valid column of a width-padded map (head_valid in the kernel source)."""
    p = torch.arange(P, device=device)
    if pitch <= wv:
        return torch.ones(P, dtype=torch.bool, device=device)
    return (p % pitch) < wv


def head_inputs(P, dtype, seed, device="cpu"):
    """y = relu(randn) rounded to dtype with about 5 % of the elements exactly 0, w ~ 0.1 randn, b = 0.3, gt = rand."""
    g = torch.Generator().manual_seed(seed)
    y = torch.relu(torch.randn(P, 64, generator=g))
    y[torch.rand(P, 64, generator=g) < 0.05] = 0.0
    w = 0.1 * torch.randn(64, generator=g)
    b = torch.tensor([0.3])
    gt = torch.rand(P, generator=g)
    return y.to(dtype).to(device), w.to(device), b.to(device), gt.to(device)


def _head_sums(d, g, y):
    """fp64 sums of the head's three reductions and the magnitude sums their bounds need."""
    terms = g[:, None] * y
    return types.SimpleNamespace(loss=(d * d).sum(), dw=terms.sum(0), db=g.sum(),
                                 loss_mag=(d * d).sum(), dw_mag=terms.abs().sum(0), db_mag=g.abs().sum())


def head_ref(y16, w, b, gt, gscale=1.0, lscale=None, pitch=0, wv=0):
    """The head in fp64: et = y.w + b, loss = sum (et - gt)^2, g = 2 (et - gt) gscale, dy = g lscale w (y > 0),
    dw = sum_p g y, db = sum g; padding columns give et = 0 and add nothing.  Also et_mag = sum_c |y w| + |b| and the
    magnitude sums dw_mag = sum_p |g y|, db_mag = sum |g|, loss_mag = sum d^2."""
    P = y16.shape[0]
    y, wd = y16.to(F64), w.to(F64)
    bd = b.to(F64).reshape(())
    valid = head_valid(P, pitch, wv, y16.device)
    zero = torch.zeros((), dtype=F64, device=y16.device)
    prod = y * wd
    et = torch.where(valid, prod.sum(1) + bd, zero)
    d = torch.where(valid, et - gt.to(F64), zero)
    g = 2.0 * d * gscale
    ls = 1.0 if lscale is None else float(lscale)
    dy = (g * ls)[:, None] * wd * (y > 0)
    r = _head_sums(d, g, y)
    r.et, r.g, r.dy, r.valid = et, g, dy, valid
    r.et_mag = prod.abs().sum(1) + bd.abs()
    return r


def head_staged(et32, y16, w, gt, gscale=1.0, lscale=None, pitch=0, wv=0):
    """What follows the kernel's own fp32 et, staged: in fp32, one rounding per operation in the kernel's order,
    d = et - gt, g = (2 d) gscale, dy = ((g lscale) w) (y > 0) rounded to y's type (the kernel has no addition there,
    so nothing can be contracted: expected bit for bit); then the fp64 sums of that fp32 g and d."""
    P = y16.shape[0]
    f32 = torch.float32
    valid = head_valid(P, pitch, wv, y16.device)
    zero = torch.zeros((), dtype=f32, device=y16.device)
    d = torch.where(valid, et32.to(f32) - gt.to(f32), zero)
    g = (2.0 * d) * torch.tensor(gscale, dtype=f32, device=y16.device)
    ls = torch.tensor(1.0 if lscale is None else float(lscale), dtype=f32, device=y16.device)
    o = (g * ls)[:, None] * w.to(f32)[None, :]
    dy = torch.where(y16 > 0, o, zero).to(y16.dtype)
    r = _head_sums(d.to(F64), g.to(F64), y16.to(F64))
    r.d, r.g, r.dy, r.valid = d, g, dy, valid
    return r


def head_chain(P, nblk):
    """The longest chain of additions one of head_train's sums goes through: a thread's pixels, the block's 32 pixel
    groups, a reduce group's blocks, the 15 groups, and the product's own rounding."""
    return math.ceil(P / (32 * nblk)) + 32 + math.ceil(nblk / REDUCE_GROUPS) + REDUCE_GROUPS + 1


def _ratio(err, bound):
    """max err / bound; an exact result is within any bound (a zero bound included)."""
    err, bound = err.to(F64).reshape(-1), bound.to(F64).reshape(-1)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return r.max().item()


def et_ratio(et, ref):
    """max |et - ref.et| / (2 * 12 * 2^-24 * (sum_c |y w| + |b|)) over the valid pixels; padding pixels must be 0."""
    bound = 2 * HEAD_ET_DEPTH * U24 * ref.et_mag
    err = (et.to(F64).reshape(-1) - ref.et).abs()
    err = torch.where(ref.valid, err, torch.where(et.reshape(-1) == 0, 0.0, float("inf")).to(F64))
    return _ratio(err, bound)


def sum_ratio(got, ref_sum, mag, P, nblk, beta=0.0, old=None):
    """max |got - (beta old + ref_sum)| / (2 L 2^-24 mag [+ 2^-23 (|beta old| + |ref_sum|)]), L = head_chain."""
    ref_sum, mag = ref_sum.to(F64).reshape(-1), mag.to(F64).reshape(-1)
    bound = 2 * head_chain(P, nblk) * U24 * mag
    want = ref_sum
    if beta != 0.0:
        bo = beta * old.to(F64).reshape(-1)
        want = bo + ref_sum
        bound = bound + 2.0 ** -23 * (bo.abs() + ref_sum.abs())
    return _ratio((got.to(F64).reshape(-1) - want).abs(), bound)


# ---------------------------------------------------------------------------------------------------------- max-pool
POOL_SHAPES = [(1, 2, 2, 8), (3, 6, 10, 24), (2, 12, 20, 64), (1, 4, 6, 128)]
# The launchers cap the grid at 8192 blocks of 256 threads = 2097152 vector items a sweep.  POOL_FULL_GRID has exactly
# that many (2 * 256 * 512 * 8): every thread takes one item and none a second.  POOL_TWO_SWEEPS has
# 2 * 256 * 514 * 8 = 2105344: the threads of the first 32 blocks take a second item, the ragged second sweep.
POOL_FULL_GRID = (2, 512, 1024, 64)
POOL_TWO_SWEEPS = (2, 512, 1028, 64)
POOL_GRID_ITEMS = 8192 * 256
_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def _windows(x):
    """[n, h, w, c] -> [n, h/2, w/2, c, 4], window position q = 2 * row + column: the scan order (0,0),(0,1),(1,0),(1,1)."""
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)


def _unwindows(v):
    n, ho, wo, c, _ = v.shape
    return v.reshape(n, ho, wo, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2 * ho, 2 * wo, c)


def pool_input(n, h, w, c, dtype, seed, negative=False, device="cpu"):
    """Post-ReLU values (negative: plain randn, so windows whose max is <= 0 occur) with, cycling over the windows:
    all four values equal, two equal maxima at each of the six position pairs, an all-zero window, (negative:) an
    all-negative window and one whose max is exactly 0 -- and one +inf, in the last of the plain random windows (the
    2 x 2 post-ReLU map has none: there it follows the two equal maxima of the (0,0),(0,1) window)."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g, device=device)
    if not negative:
        x = torch.relu(x)
    v = _windows(x).clone()
    flat = v.reshape(-1, 4)
    # (negative: the cycle starts at the all-negative window, so that the 2 x 2 map's 8 windows hold both of its kinds)
    kind = (torch.arange(flat.shape[0], device=device) + (8 if negative else 0)) % 16
    flat[kind == 0] = 1.5
    for k, (a, b) in enumerate(_PAIRS):
        pat = torch.full((4,), 0.25, device=device)
        pat[a] = 2.0
        pat[b] = 2.0
        flat[kind == 1 + k] = pat
    flat[kind == 7] = 0.0
    if negative:
        flat[kind == 8] = torch.tensor([-1.0, -0.5, -2.0, -0.5], device=device)
        flat[kind == 9] = torch.tensor([-1.0, 0.0, -2.0, 0.0], device=device)
    plain = torch.nonzero(kind >= 10)
    flat[int(plain[-1]) if plain.numel() else 1, 2] = float("inf")
    return _unwindows(flat.reshape(v.shape)).to(dtype).contiguous()


def pack_codes(nib):
    """[..., c] 4-bit values -> int32 [..., c / 8]: channel c in word c // 8, nibble c % 8."""
    c = nib.shape[-1]
    v = nib.to(torch.int64).reshape(*nib.shape[:-1], c // 8, 8)
    sh = 4 * torch.arange(8, device=nib.device)
    word = (v << sh).sum(-1)
    word = torch.where(word >= 2 ** 31, word - 2 ** 32, word)
    return word.to(torch.int32)


def unpack_codes(codes):
    """int32 [..., c / 8] -> int64 [..., c] nibbles."""
    word = codes.to(torch.int64) & 0xFFFFFFFF
    sh = 4 * torch.arange(8, device=codes.device)
    nib = (word[..., None] >> sh) & 0xF
    return nib.reshape(*codes.shape[:-1], codes.shape[-1] * 8)


def maxpool_ref(x):
    """nn.MaxPool2d(2, 2) on NHWC by an explicit scan of each window in order (0,0),(0,1),(1,0),(1,1) with strict '>':
    the first max wins.  Returns (pooled [n,h/2,w/2,c] in x's type, codes int32 [n,h/2,w/2,c/8], route bool [n,h,w,c]):
    the code is the one-hot of the first max's position, 0 when that max is not > 0, and route marks the one element
    of each window the backward hands the pooled gradient to (none where the code is 0).  Comparisons of 16-bit values
    are exact in fp32, which is what this scans in."""
    v = _windows(x.float())
    best = v[..., 0].clone()
    arg = torch.zeros(best.shape, dtype=torch.int64, device=x.device)
    for q in (1, 2, 3):
        better = v[..., q] > best
        best = torch.where(better, v[..., q], best)
        arg = torch.where(better, torch.full_like(arg, q), arg)
    pos = best > 0
    nib = torch.where(pos, torch.ones_like(arg) << arg, torch.zeros_like(arg))
    onehot = (torch.arange(4, device=x.device) == arg[..., None]) & pos[..., None]
    return best.to(x.dtype), pack_codes(nib), _unwindows(onehot)


def maxpool_route(route, dy):
    """The backward: dx = dy of the window at the routed element, 0 elsewhere."""
    up = dy.repeat_interleave(2, 1).repeat_interleave(2, 2)
    return torch.where(route, up, torch.zeros((), dtype=dy.dtype, device=dy.device))


# ---------------------------------------------------------------------------------------------------------- split_x3
# (C, stride, mode): the float4 kernel (dense, C % 4 == 0) and the general one (small, padded or strided C)
SPLIT_VEC = [(4, 12, 0), (4, 4, 1), (64, 192, 0), (64, 64, 1)]
SPLIT_GENERAL = [(3, 64, 0), (6, 8, 1), (64, 72, 1)]
SPLIT_M = [1, 37, 5000]
SPLIT_PATTERNS = [0, 0b100, 0b010, 0b111]


def split_input(M, C, seed, device="cpu"):
    """fp32 [M, C]: randn with values that are exact in bf16 (lo = 0), 1e30 and 1e-30 spread over it."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M * C, generator=g)
    i = torch.arange(M * C)
    x[i % 5 == 1] = x[i % 5 == 1].to(torch.bfloat16).float()
    x[i % 11 == 3] = 1e30
    x[i % 13 == 5] = 1e-30
    x[i % 17 == 7] = -1e30
    return x.reshape(M, C).to(device)


def split_x3_ref(x, mode, pattern, stride):
    """x fp32 [M, C] -> bf16: hi = bf16(x), lo = bf16(x - hi); block b of three is lo if bit b of pattern is set, else
    hi.  mode 0: [M, stride], block b at channels [b C, (b + 1) C), zero from 3 C on; mode 1: [3, M, stride], block b
    the b-th slab, zero from C on."""
    M, C = x.shape
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    blocks = [lo if (pattern >> b) & 1 else hi for b in range(3)]
    if mode == 0:
        out = torch.zeros(M, stride, dtype=torch.bfloat16, device=x.device)
        for b in range(3):
            out[:, b * C:(b + 1) * C] = blocks[b]
    else:
        out = torch.zeros(3, M, stride, dtype=torch.bfloat16, device=x.device)
        for b in range(3):
            out[b, :, :C] = blocks[b]
    return out


# -------------------------------------------------------------------------------------------------------- loss scale
def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def loss_scale_ref(S, n, overflow, interval, growth, backoff, max_scale):
    """One step of the scaler {S, 1/S, clean steps} in Python floats rounded to fp32 after every operation: on overflow
    S = max(S backoff, 1) and the count restarts; after ``interval`` clean steps S = min(S growth, max_scale) and the
    count restarts; else the count advances.  Returns (S, 1/S, n)."""
    S, n = _f32(S), _f32(n)
    if overflow:
        S, n = max(_f32(S * _f32(backoff)), 1.0), 0.0
    elif _f32(n + 1.0) >= float(interval):
        S, n = min(_f32(S * _f32(growth)), _f32(max_scale)), 0.0
    else:
        n = _f32(n + 1.0)
    return S, _f32(1.0 / S), n


SCALER_ARGS = dict(interval=3, growth=2.0, backoff=0.5, max_scale=65536.0)
# name -> (start S, start n, [(overflow flag, expected (S, 1/S, n) after the launch)]): the expected states are written
# out by hand for interval 3, growth 2, backoff 0.5, max_scale 65536
SCALER_TRANSITIONS = {
    "growth_at_interval": (1.0, 0.0, [(0, (1.0, 1.0, 1.0)), (0, (1.0, 1.0, 2.0)), (0, (2.0, 0.5, 0.0))]),
    "growth_capped": (32768.0, 2.0, [(0, (65536.0, 2.0 ** -16, 0.0)), (0, (65536.0, 2.0 ** -16, 1.0)),
                                     (0, (65536.0, 2.0 ** -16, 2.0)), (0, (65536.0, 2.0 ** -16, 0.0))]),
    "backoff": (1024.0, 1.0, [(1, (512.0, 2.0 ** -9, 0.0))]),
    "backoff_floored": (1.0, 0.0, [(1, (1.0, 1.0, 0.0))]),
    "counter_reset": (2.0, 2.0, [(1, (1.0, 1.0, 0.0)), (0, (1.0, 1.0, 1.0)), (0, (1.0, 1.0, 2.0)),
                                 (0, (2.0, 0.5, 0.0))]),
    # one run of 14 launches from S = 1 through all of the above
    "sequence": (1.0, 0.0, [
        (1, (1.0, 1.0, 0.0)),            # backoff floored at 1
        (0, (1.0, 1.0, 1.0)),
        (0, (1.0, 1.0, 2.0)),
        (0, (2.0, 0.5, 0.0)),            # growth at the interval
        (0, (2.0, 0.5, 1.0)),
        (1, (1.0, 1.0, 0.0)),            # backoff, the count of 1 dropped
        (0, (1.0, 1.0, 1.0)),
        (0, (1.0, 1.0, 2.0)),
        (0, (2.0, 0.5, 0.0)),
        (0, (2.0, 0.5, 1.0)),
        (0, (2.0, 0.5, 2.0)),
        (0, (4.0, 0.25, 0.0)),
        (1, (2.0, 0.5, 0.0)),            # backoff above the floor
        (1, (1.0, 1.0, 0.0)),
    ]),
}
