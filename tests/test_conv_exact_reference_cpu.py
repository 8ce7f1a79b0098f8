"""tests/conv_exact_reference.py against independent code, on the CPU: the shifted-sum references against F.conv2d and
autograd in float64, the pool-backward and code references against tests/elementwise_reference.py, the operand ranges of
every GPU test family against the three conditions the exact comparison rests on (bound below 2^24, outputs that need
rounding, exact ties), and -- once -- the gap the exact comparison closes: one term removed from a weight gradient over
262144 pixels passes numerics.check_sum32 and fails torch.equal.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_reference as R
from elementwise_reference import maxpool_ref, maxpool_route, unpack_codes
from numerics import check_sum32

F64 = torch.float64
DTYPES = [torch.bfloat16, torch.float16]
# (n, h, w, ci, co, ksize, dil): 3x3 at dilation 1 and 2, 1x1, N > 1, maps smaller than the dilated kernel
SHAPES = [(1, 5, 6, 4, 6, 3, 1), (2, 7, 5, 8, 4, 3, 2), (2, 4, 6, 8, 8, 1, 1), (3, 1, 4, 4, 4, 3, 1),
          (1, 3, 2, 4, 8, 3, 2), (2, 1, 1, 8, 4, 3, 1)]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _operands(n, h, w, ci, co, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, h, w, ci, generator=g, dtype=F64), torch.randn(co, ci, k, k, generator=g, dtype=F64),
            torch.randn(co, generator=g, dtype=F64), torch.randn(n, h, w, co, generator=g, dtype=F64))


# ------------------------------------------------------------------------------------------- against independent code
@pytest.mark.parametrize("n,h,w,ci,co,k,dil", SHAPES)
def test_forward_matches_conv2d(n, h, w, ci, co, k, dil):
    x, wt, b, _ = _operands(n, h, w, ci, co, k)
    pad = dil * (k // 2)
    y = _nhwc(F.conv2d(_nchw(x), wt, b, padding=pad, dilation=dil))
    torch.testing.assert_close(R.conv_fwd_ref(x, wt, b, dil, "bias"), y, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.conv_fwd_ref(x, wt, b, dil), torch.relu(y), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.conv_fwd_ref(x, wt, b, dil, "none"), y - b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("n,h,w,ci,co,k,dil", SHAPES)
def test_gradients_match_autograd(n, h, w, ci, co, k, dil):
    x, wt, b, dy = _operands(n, h, w, ci, co, k, seed=1)
    xr, wr, br = _nchw(x).clone().requires_grad_(), wt.clone().requires_grad_(), b.clone().requires_grad_()
    y = F.conv2d(xr, wr, br, padding=dil * (k // 2), dilation=dil)
    gx, gw, gb = torch.autograd.grad(y, (xr, wr, br), _nchw(dy))
    torch.testing.assert_close(R.dgrad_ref(dy, wt, dil), _nhwc(gx), rtol=1e-12, atol=1e-12)
    dw, db = R.wgrad_ref(dy, x, k, dil)
    torch.testing.assert_close(dw, gw, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db, gb, rtol=1e-12, atol=1e-12)
    mask = torch.randn(n, h, w, ci, dtype=F64)
    torch.testing.assert_close(R.dgrad_mask_ref(dy, wt, mask, dil), _nhwc(gx) * (mask > 0), rtol=1e-12, atol=1e-12)
    dw0 = torch.randn_like(gw)
    torch.testing.assert_close(R.wgrad_update_ref(dw, dw0, 0.5, 0.25, 2.0 ** -3), 0.5 * dw0 + 2.0 ** -5 * gw,
                               rtol=1e-12, atol=1e-12)
    assert torch.equal(R.wgrad_update_ref(dw, dw0, 0.0, 1.0), dw)


def test_first_layer_matches_conv2d():
    g = torch.Generator().manual_seed(2)
    x4 = torch.randn(2, 6, 7, 4, generator=g, dtype=F64)
    x4[..., 3] = 0
    wt, b = torch.randn(8, 3, 3, 3, generator=g, dtype=F64), torch.randn(8, generator=g, dtype=F64)
    dy = torch.randn(2, 6, 7, 8, generator=g, dtype=F64)
    xr, wr, br = _nchw(x4[..., :3]).clone(), wt.clone().requires_grad_(), b.clone().requires_grad_()
    y = F.conv2d(xr, wr, br, padding=1)
    torch.testing.assert_close(R.conv_first_ref(x4, wt, b), torch.relu(_nhwc(y)).detach(), rtol=1e-12, atol=1e-12)
    gw, gb = torch.autograd.grad(y, (wr, br), _nchw(dy))
    dw, db = R.wgrad_first_ref(dy, x4)
    torch.testing.assert_close(dw, gw, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db, gb, rtol=1e-12, atol=1e-12)


def test_integer_operands_are_summed_exactly():
    """With the generators' operands the fp64 references equal conv2d bit for bit: no rounding anywhere."""
    _, x = R.int_operand((2, 6, 7, 64), R.X_ACT, torch.bfloat16, 3)
    _, wt = R.int_operand((64, 64, 3, 3), R.W_FWD, torch.float16, 4)
    _, b = R.int_operand((64,), R.B_FWD, torch.float32, 5)
    y = _nhwc(F.conv2d(_nchw(x), wt, b, padding=2, dilation=2))
    assert torch.equal(R.conv_fwd_ref(x, wt, b, 2, "bias"), y)
    assert R.exactness_bound(lambda a, c, d: R.conv_fwd_ref(a, c, d, 2, "bias"), (x, wt, b), 6) < R.LIMIT


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_references_match_elementwise_reference(dtype):
    """poolbwd_ref (decoded from the codes) == maxpool_route of maxpool_ref's route; pool_fwd_ref's pooled map and
    codes are maxpool_ref's of the rounded full map, and the pooled map is ATen's max-pool of it."""
    full16, _ = R.relu_operand((2, 6, 8, 16), R.POOL_MAP, dtype, 6)
    _, codes, route = maxpool_ref(full16)
    assert int((unpack_codes(codes) == 0).sum()) > 0               # all-zero windows occur: code 0, no gradient
    _, d = R.int_operand((2, 3, 4, 16), R.X_ACT, dtype, 7)
    assert torch.equal(R.poolbwd_ref(d, codes), maxpool_route(route, d))
    assert int((R.poolbwd_ref(d.abs() + 1, codes) != 0).sum()) == int(route.sum())

    x16, x = R.int_operand((2, 6, 8, 64), R.X_ACT, dtype, 8)
    _, wt = R.int_operand((16, 64, 3, 3), R.W_FWD, dtype, 9)
    _, b = R.int_operand((16,), R.B_FWD, torch.float32, 10)
    full, pooled, codes2 = R.pool_fwd_ref(x, wt, b, dtype)
    assert full.dtype == dtype and torch.equal(full, R.to16(R.conv_fwd_ref(x, wt, b), dtype))
    p2, c2, _ = maxpool_ref(full)
    assert torch.equal(pooled, p2) and torch.equal(codes2, c2)
    assert torch.equal(pooled.float(), _nhwc(F.max_pool2d(_nchw(full.float()), 2)))


# ------------------------------------------------------------------------------------------------ rounding machinery
@pytest.mark.parametrize("dtype", DTYPES)
def test_rounding_stats_and_to16(dtype):
    p = R.MANT[dtype]
    one_ulp = 2.0 ** (1 - p)                               # spacing in [1, 2)
    v = torch.tensor([1.0, 1.0 + one_ulp, 1.0 + one_ulp / 2, 1.0 + 3 * one_ulp / 2, 1.0 + one_ulp / 4, 0.0,
                      -(2.0 + one_ulp), 2.0 - one_ulp / 2], dtype=F64)
    share, ties = R.rounding_stats(v, dtype)
    assert ties == 4 and share == 5 / 7                    # the two ties in [1, 2), -(2 + half a spacing), 2 - ...
    r = R.to16(v, dtype).to(F64)
    # round half to even: 1 + ulp/2 -> 1 (even), 1 + 3 ulp/2 -> 1 + 2 ulp (even)
    assert r[2] == 1.0 and r[3] == 1.0 + 2 * one_ulp and r[6] == -2.0 and r[7] == 2.0
    with pytest.raises(AssertionError):
        R.to16(torch.tensor([1.0 + 2.0 ** -30], dtype=F64), dtype)     # not an fp32 value: the bound was not held
    with pytest.raises(AssertionError):
        R.int_operand((4,), (257, 257, 0), torch.bfloat16, 0)            # 257 needs 9 bits


# ------------------------------------------------------------------ the operand ranges of the GPU test families
def _fwd_family(ci, k, dil, dtype, density=1.0, wrng=R.W_FWD, m=(2, 12, 16)):
    _, x = R.int_operand((*m, ci), R.X_ACT, dtype, 11, density=density)
    _, wt = R.int_operand((64, ci, k, k), wrng, dtype, 12, density=density)
    _, b = R.int_operand((64,), R.B_FWD, torch.float32, 13)
    return x, wt, b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci,k,dil", [(64, 1, 1), (1024, 3, 2)])
def test_forward_family_ranges(ci, k, dil, dtype):
    """Forward / data-gradient families at their smallest (1x1, Cin 64) and largest (3x3, Cin 1024) K."""
    x, wt, b = _fwd_family(ci, k, dil, dtype)
    bound = R.exactness_bound(lambda a, c, d: R.conv_fwd_ref(a, c, d, dil, "bias"), (x, wt, b), R.W_FWD[2])
    share, ties = R.rounding_stats(R.conv_fwd_ref(x, wt, b, dil), dtype)
    print(f"\nfwd K={k * k * ci} {dtype}: bound {bound:.4g} share {share:.3f} ties {ties}")
    assert bound < R.LIMIT and share >= 0.01 and ties >= 8
    # the hard upper limit of the ranges at the largest K of the model
    assert 9 * 1024 * 12 * 32 + 16 * 16 < R.LIMIT


@pytest.mark.parametrize("dtype", DTYPES)
def test_first_layer_family_ranges(dtype):
    x4 = torch.zeros(2, 12, 16, 4, dtype=F64)
    x4[..., :3] = R.int_operand((2, 12, 16, 3), R.X_FIRST, dtype, 14)[1]
    _, wt = R.int_operand((64, 3, 3, 3), R.W_FWD, dtype, 15)
    _, b = R.int_operand((64,), R.B_FWD, torch.float32, 16)
    bound = R.exactness_bound(R.conv_first_ref, (x4, wt, b), R.W_FWD[2])
    share, ties = R.rounding_stats(R.conv_first_ref(x4, wt, b), dtype)
    print(f"\nfirst layer {dtype}: bound {bound:.4g} share {share:.3f} ties {ties}")
    assert bound < R.LIMIT and share >= 0.01 and ties >= 8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,k", [((129, 2, 4), 9 * 64), ((2, 16, 96), 9 * 128), ((2, 8, 64), 9 * 512)])
def test_bias_partial_family_ranges(m, k, dtype):
    """Bias partials sum every pixel of a channel, so the operands are sparse (sparse_density) with a wide weight range:
    few, large terms keep the per-channel bound below 2^24 while the gradient values still need rounding (a partial
    that summed the rounded values would differ)."""
    ci = k // 9
    M = m[0] * m[1] * m[2]
    dens = R.sparse_density(k, M)
    x, wt, _ = _fwd_family(ci, 3, 1, dtype, density=dens, wrng=R.W_BP, m=m)
    bound = R.bias_partial_bound(lambda a, c: R.conv_ref(a, c, 1), (x, wt), R.W_BP[2])
    share, ties = R.rounding_stats(R.conv_ref(x, wt, 1), dtype)
    print(f"\nbias partials M={M} K={k} {dtype}: density {dens:.3f} bound {bound:.4g} share {share:.3f} ties {ties}")
    assert bound < R.LIMIT and share >= 0.01 and ties >= 8


@pytest.fixture(scope="module")
def wgrad_262144():
    """The M = 262144 weight gradient of the halo / ring kernels' threshold (64 -> 64), once for the tests below."""
    _, x = R.int_operand((1, 256, 1024, 64), R.X_WG, torch.bfloat16, 17)
    _, dy = R.int_operand((1, 256, 1024, 64), R.X_WG, torch.bfloat16, 18)
    dw, db = R.wgrad_ref(dy, x, 3, 1)
    return x, dy, dw, db


def test_weight_gradient_family_ranges(wgrad_262144):
    """Weight gradients are fp32 outputs: nothing is rounded, the bound is the whole condition.  Smallest M and the
    largest (262144, where cfg 8 starts)."""
    x, dy, dw, db = wgrad_262144
    assert 262144 * 3 * 3 < R.LIMIT                       # whatever the draw
    assert R.exactness_bound(lambda a, c: R.wgrad_ref(a, c, 3, 1), (dy, x), 0) < R.LIMIT
    R.to32(dw), R.to32(db)
    _, xs = R.int_operand((1, 3, 2, 64), R.X_WG, torch.float16, 19)
    _, ds = R.int_operand((1, 3, 2, 64), R.X_WG, torch.float16, 20)
    assert R.exactness_bound(lambda a, c: R.wgrad_ref(a, c, 3, 2), (ds, xs), 0) < R.LIMIT
    # beta / scale / dscale: dw0 integers, beta 0.5, scale 0.25, dscale 2^-3 -> units of 2^-5
    _, dw0 = R.int_operand(tuple(dw.shape), (-64, 64, 0), torch.float32, 21)
    R.to32(R.wgrad_update_ref(dw, dw0, 0.5, 0.25, 2.0 ** -3))
    assert (float(dw.abs().max()) + 64) * 2.0 ** 5 < R.LIMIT


def test_one_missing_term_passes_check_sum32_and_fails_equal(wgrad_262144):
    """The gap, recorded once.  A weight gradient over M = 262144 pixels with one product removed from one element:
    with N(0, 1) operands (tests/test_gpu_conv.py) the elements have a standard deviation of sqrt(M) = 512, check_sum32
    allows 1e-3 (max|ref| + |ref|), about 2, and the missing term is about 1 -- accepted.  With the exact operands the
    same defect is a difference of an integer and torch.equal refuses it."""
    x, dy, dw, _ = wgrad_262144
    g = torch.Generator().manual_seed(22)
    xn = torch.randn(262144, 64, generator=g).to(torch.bfloat16).float()
    dn = torch.randn(262144, 64, generator=g).to(torch.bfloat16).float()
    ref = dn.t() @ xn                                     # the centre tap's [Co][Ci] plane
    t = (dn[:, 5] * xn[:, 7]).abs()
    m = int(torch.argmax(((t > 0.5) & (t <= 1.0)).to(torch.int8)))      # a typical term (0.5 < |term| <= 1)
    term = float(dn[m, 5] * xn[m, 7])
    assert term != 0.0
    wrong = ref.clone()
    wrong[5, 7] -= term
    assert 300 < float(ref.std()) < 800
    check_sum32(wrong, ref)                               # passes: the defect is invisible

    xm, dm = x.reshape(-1, 64), dy.reshape(-1, 64)
    m = int(torch.argmax(((dm[:, 5] * xm[:, 7]) != 0).to(torch.int8)))
    exact = R.to32(dw[:, :, 1, 1])
    wrong = exact.clone()
    wrong[5, 7] -= float(dm[m, 5] * xm[m, 7])
    assert not torch.equal(wrong, exact)
