"""Stride-2 convolutions (csrc/conv_stride2.hip; the down-sampling conv and the 2x transposed conv, k = 1 .. 4, Ci and
Co any multiples of 16): bit for bit against fp64 references with the exactly representable operands of
tests/conv_exact_reference.py (asserted bound < 2^24, ``torch.equal``, no tolerance), the public ops against fp32 ATen
with the thresholds of tests/test_library_ops.py, the weight gradient's repeatability, opcheck / torch.compile, and
the refusals.  The references are strided slices of a zero-padded map times matmuls, one per tap."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_exact_reference as R
from can_distributed_pytorch_amd.ops import library as L

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
# ci, co, k, small map (n, h, w) (the large map is (n, 2h, 2w)), forward epilogue, beta of the weight gradient
CASES = [
    (16, 16, 1, (1, 1, 1), "bias_relu", 0.0),
    (16, 16, 2, (1, 1, 1), "bias", 1.0),
    (16, 16, 3, (1, 1, 1), "bias_relu", 0.0),         # one small pixel, kernel wider than the map
    (16, 32, 4, (1, 1, 3), "bias", 1.0),
    (48, 32, 3, (2, 5, 1), "none", 0.0),              # one column, a 16-channel tail, one row past a 4-row tile
    (32, 48, 4, (1, 9, 33), "bias_relu", 1.0),        # one row and one column past a tile (4 x 32 and 8 x 32)
    (80, 96, 2, (1, 17, 35), "bias", 0.0),            # three chunks with tail, two passes
    (64, 64, 3, (1, 8, 32), "bias_relu", 0.0),        # whole tiles only, both multiples of 64
    (160, 16, 4, (2, 8, 32), "none", 1.0),
    (16, 80, 3, (3, 9, 11), "bias_relu", 1.0),        # four blocks + one
    (128, 64, 1, (1, 16, 65), "bias", 0.0),
    (128, 64, 4, (1, 16, 65), "bias", 0.0)]           # several weight-gradient slices
EPI = {"bias_relu": "EPI_BIAS_RELU", "bias": "EPI_BIAS", "none": "EPI_NONE"}


def _conv():
    from can_distributed_pytorch_amd.ops import conv as C
    return C


def _padded(big, k):
    """The large map with (k - 1) // 2 zeros before and enough after: tap (kh, kw) of small pixel (i, j) is
    [2 i + kh, 2 j + kw]."""
    n, h, w, c = big.shape
    p = (k - 1) // 2
    out = torch.zeros(n, h + k, w + k, c, dtype=big.dtype, device=big.device)
    out[:, p:p + h, p:p + w] = big
    return out


def down_ref(x, w):
    """y[n, i, j, co] = sum x[n, 2 i - p + kh, 2 j - p + kw, ci] w[co, ci, kh, kw]  (fp64)."""
    n, h, wd, ci = x.shape
    co, _, k, _ = w.shape
    xp, y = _padded(x, k), torch.zeros(n * (h // 2) * (wd // 2), co, dtype=R.F64, device=x.device)
    for kh in range(k):
        for kw in range(k):
            y += xp[:, kh:kh + h:2, kw:kw + wd:2].reshape(-1, ci) @ w[:, :, kh, kw].t()
    return y.reshape(n, h // 2, wd // 2, co)


def up_ref(x, wt):
    """y[n, 2 i - p + kh, 2 j - p + kw, co] += x[n, i, j, ci] wt[ci, co, kh, kw]  (fp64)."""
    n, h, wd, ci = x.shape
    _, co, k, _ = wt.shape
    p = (k - 1) // 2
    yp = torch.zeros(n, 2 * h + k, 2 * wd + k, co, dtype=R.F64, device=x.device)
    for kh in range(k):
        for kw in range(k):
            yp[:, kh:kh + 2 * h:2, kw:kw + 2 * wd:2] += x @ wt[:, :, kh, kw]
    return yp[:, p:p + 2 * h, p:p + 2 * wd].contiguous()


def s2_wgrad_ref(small, big, k):
    """(dw[a, b, kh, kw] = sum small[n, i, j, a] big[n, 2 i - p + kh, 2 j - p + kw, b], pixel sums of small, of big)."""
    n, h, wd, ca = small.shape
    cb = big.shape[-1]
    bp, s2 = _padded(big, k), small.reshape(-1, ca).t().contiguous()
    dw = torch.zeros(ca, cb, k, k, dtype=R.F64, device=small.device)
    for kh in range(k):
        for kw in range(k):
            dw[:, :, kh, kw] = s2 @ bp[:, kh:kh + 2 * h:2, kw:kw + 2 * wd:2].reshape(-1, cb)
    return dw, s2.sum(1), big.reshape(-1, cb).sum(0)


def epilogue_ref(y, b, epi):
    if epi == "none":
        return y
    return torch.relu(y + b) if epi == "bias_relu" else y + b


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci,co,k,nhw,epi,beta", CASES)
def test_forward_and_dgrad_exact(ci, co, k, nhw, epi, beta, dtype):
    C = _conv()
    n, h, w = nhw
    big = (n, 2 * h, 2 * w)
    xb16, xb = R.int_operand((*big, ci), R.X_ACT, dtype, 1, DEV)        # down's input
    xs16, xs = R.int_operand((*nhw, ci), R.X_ACT, dtype, 2, DEV)        # up's input
    gs16, gs = R.int_operand((*nhw, co), R.X_ACT, dtype, 3, DEV)        # down's dY
    gb16, gb = R.int_operand((*big, co), R.X_ACT, dtype, 4, DEV)        # up's dY
    wd16, wd = R.int_operand((co, ci, k, k), R.W_FWD, dtype, 5, DEV)    # down's weight
    wu16, wu = R.int_operand((ci, co, k, k), R.W_FWD, dtype, 6, DEV)    # up's weight
    b32, b = R.int_operand((co,), R.B_FWD, torch.float32, 7, DEV)
    shift = R.W_FWD[2]
    for ref, ops in ((down_ref, (xb, wd)), (up_ref, (gs, wd)), (up_ref, (xs, wu)), (down_ref, (gb, wu))):
        assert R.exactness_bound(ref, ops, shift) + 16 * 2.0 ** (shift - R.B_FWD[2]) < R.LIMIT      # + |bias|
    code, bias = getattr(C, EPI[epi]), (None if epi == "none" else b32)
    y_down = C.conv_down2(xb16, C.pack_weight_fwd(wd16.float(), dtype), bias, ksize=k, epi=code)
    dx_down = C.conv_up2(gs16, C.pack_weight_up(wd16.float(), dtype), None, ksize=k, epi=C.EPI_NONE)
    y_up = C.conv_up2(xs16, C.pack_weight_up(wu16.float(), dtype), bias, ksize=k, epi=code)
    dx_up = C.conv_down2(gb16, C.pack_weight_fwd(wu16.float(), dtype), None, ksize=k, epi=C.EPI_NONE)
    torch.cuda.synchronize()
    assert torch.equal(y_down, R.to16(epilogue_ref(down_ref(xb, wd), b, epi), dtype))
    assert torch.equal(dx_down, R.to16(up_ref(gs, wd), dtype))
    assert torch.equal(y_up, R.to16(epilogue_ref(up_ref(xs, wu), b, epi), dtype))
    assert torch.equal(dx_up, R.to16(down_ref(gb, wu), dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bias_of", ["small", "big"])
@pytest.mark.parametrize("ci,co,k,nhw,epi,beta", CASES)
def test_wgrad_exact(ci, co, k, nhw, epi, beta, bias_of, dtype):
    C = _conv()
    n, h, w = nhw
    # down (bias_of small): small = dY [.., co], big = x [.., ci]; up (bias_of big): small = x [.., ci], big = dY [.., co]
    ca, cb = (co, ci) if bias_of == "small" else (ci, co)
    s16, s = R.int_operand((*nhw, ca), R.X_WG, dtype, 8, DEV)
    b16, bg = R.int_operand((n, 2 * h, 2 * w, cb), R.X_WG, dtype, 9, DEV)
    dw, dw0 = R.int_operand((ca, cb, k, k), R.X_ACT, torch.float32, 10, DEV)
    db, db0 = R.int_operand((co,), R.X_ACT, torch.float32, 11, DEV)
    assert R.exactness_bound(lambda a, c: s2_wgrad_ref(a, c, k), (s, bg), 0) * 2 + 12 < R.LIMIT   # scale 2, |dw0| <= 12
    C.conv_s2_wgrad(s16, b16, dw, db if epi != "none" else None, ksize=k, bias_of=bias_of, beta=beta, scale=2.0)
    torch.cuda.synchronize()
    rw, rsmall, rbig = s2_wgrad_ref(s, bg, k)
    rb = rsmall if bias_of == "small" else rbig
    assert torch.equal(dw, R.to32(R.wgrad_update_ref(rw, dw0, beta, 2.0)))
    assert torch.equal(db, R.to32(R.wgrad_update_ref(rb, db0, beta, 2.0) if epi != "none" else db0))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("up,ci,co,k", [(False, 32, 48, 3), (False, 64, 64, 1), (True, 48, 32, 2), (True, 64, 64, 4)])
def test_public_ops_vs_aten(up, ci, co, k, dtype):
    rel = lambda a, b: ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()  # noqa: E731
    torch.manual_seed(0)
    p = (k - 1) // 2
    x = torch.randn(2, *((10, 19) if up else (20, 38)), ci, device=DEV).to(dtype)
    m = (L.ConvTranspose2dUp2NHWC if up else L.Conv2dDown2NHWC)(ci, co, k).cuda()
    with torch.no_grad():
        m.weight.normal_(0, 0.05)
        m.bias.normal_(0, 0.1)
        m.weight.copy_(m.weight.to(dtype).float())               # the reference sees the 16-bit-rounded weights
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wr, br = m.weight.detach().clone().requires_grad_(True), m.bias.detach().clone().requires_grad_(True)
    z = F.conv_transpose2d(xr, wr, br, stride=2, padding=p, output_padding=k % 2) if up else \
        F.conv2d(xr, wr, br, stride=2, padding=p)
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    assert y.dtype == dtype and y.shape == (2, 20 if up else 10, 38 if up else 19, co)
    assert rel(y.float().permute(0, 3, 1, 2), F.relu(z)) < 1e-2
    g = torch.randn_like(z)
    y.backward(g.permute(0, 2, 3, 1).to(dtype))
    dz = g.to(dtype).float() * (y.float().permute(0, 3, 1, 2) > 0)     # the op's own ReLU mask, as test_library_ops
    refs = torch.autograd.grad(z, [xr, wr, br], dz)
    assert rel(xg.grad.float().permute(0, 3, 1, 2), refs[0]) < 1e-2
    assert rel(m.weight.grad, refs[1]) < 1e-2
    assert rel(m.bias.grad, refs[2]) < 1e-2


@pytest.mark.gpu
def test_wgrad_repeatable():
    C = _conv()
    torch.manual_seed(0)
    small = torch.randn(2, 40, 70, 48, device=DEV).to(torch.bfloat16)
    big = torch.randn(2, 80, 140, 32, device=DEV).to(torch.bfloat16)
    from can_distributed_pytorch_amd.ops import _ext
    assert _ext.require().conv_s2_slices(2 * 40 * 70, 48, 32) > 1
    outs = []
    for _ in range(2):
        dw, db = torch.empty(48, 32, 3, 3, device=DEV), torch.empty(32, device=DEV)
        C.conv_s2_wgrad(small, big, dw, db, ksize=3, bias_of="big")
        outs.append((dw, db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.gpu
def test_opcheck_and_compile():
    x = torch.randn(1, 8, 16, 32, device=DEV).to(torch.bfloat16)
    b = torch.randn(48, device=DEV)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.cannet.conv2d_down2_nhwc.default,
                          (x, torch.randn(48, 32, 3, 3, device=DEV) * 0.05, b, True), test_utils=utils)
    torch.library.opcheck(torch.ops.cannet.conv_transpose2d_up2_nhwc.default,
                          (x, torch.randn(32, 48, 4, 4, device=DEV) * 0.05, b, True), test_utils=utils)
    m = nn.Sequential(L.Conv2dDown2NHWC(32, 48, 3), L.ConvTranspose2dUp2NHWC(48, 16, 2)).cuda()
    assert torch.equal(torch.compile(m, fullgraph=True, backend="aot_eager")(x), m(x))


def test_shapes_and_refusals_cpu():
    from torch._subclasses.fake_tensor import FakeTensorMode
    ops = torch.ops.cannet
    with FakeTensorMode():
        x = torch.empty(2, 24, 32, 32, dtype=torch.bfloat16)
        wd, wu, b = torch.empty(48, 32, 3, 3), torch.empty(32, 48, 4, 4), torch.empty(48)
        y = ops.conv2d_down2_nhwc(x, wd, b, True)
        assert y.shape == (2, 12, 16, 48) and y.dtype == torch.bfloat16
        z = ops.conv_transpose2d_up2_nhwc(x, wu, b, True)
        assert z.shape == (2, 48, 64, 48) and z.dtype == torch.bfloat16
        for got, w_, need_bias in ((ops.conv2d_down2_nhwc_backward(y, x, y, wd, True, True), wd, 48),
                                   (ops.conv_transpose2d_up2_nhwc_backward(z, x, z, wu, True, False), wu, 0)):
            assert got[0].shape == x.shape and got[0].dtype == torch.bfloat16
            assert got[1].shape == w_.shape and got[1].dtype == torch.float32 and got[2].shape == (need_bias,)
        bad = [(torch.empty(2, 23, 32, 32, dtype=torch.bfloat16), wd),      # odd H
               (torch.empty(2, 24, 31, 32, dtype=torch.bfloat16), wd),      # odd W
               (x, torch.empty(48, 32, 5, 5)),                              # k = 5
               (torch.empty(2, 24, 32, 24, dtype=torch.bfloat16), torch.empty(48, 24, 3, 3)),   # Ci = 24
               (torch.empty(2, 24, 32, 32), wd)]                            # fp32 x
        for xb, w_ in bad:
            with pytest.raises(ValueError):
                ops.conv2d_down2_nhwc(xb, w_, b, True)
        for xb, w_ in bad[2:]:
            with pytest.raises(ValueError):
                ops.conv_transpose2d_up2_nhwc(xb, w_.transpose(0, 1), b, True)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_module_state_dicts_cpu(k):
    p = (k - 1) // 2
    pairs = [(L.Conv2dDown2NHWC(32, 48, k), nn.Conv2d(32, 48, k, stride=2, padding=p)),
             (L.ConvTranspose2dUp2NHWC(32, 48, k), nn.ConvTranspose2d(32, 48, k, stride=2, padding=p,
                                                                      output_padding=k % 2))]
    for ours, stock in pairs:
        assert {n: v.shape for n, v in ours.state_dict().items()} == {n: v.shape for n, v in stock.state_dict().items()}
        ours.load_state_dict(stock.state_dict())
