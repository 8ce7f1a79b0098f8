"""Thin convolutions (csrc/conv_thin.hip; one channel count 1 .. 8, the other a multiple of 16): bit for bit against the
fp64 references of tests/conv_exact_reference.py with exactly representable operands (asserted bound < 2^24,
``torch.equal``, no tolerance), through the public op against fp32 ATen with the threshold of
tests/test_gpu_conv_small.py, opcheck / torch.compile, the weight gradient's repeatability, and the refusals."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_reference as R
from can_distributed_pytorch_amd.ops import library as L

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
# ci, co, k, dil, (n, h, w), forward epilogue, beta of the weight gradient.  The pixel tile is 8 x 32: (1,17,35),
# (1,16,65), (2,8,33) are one pixel past it; (1,9,11) with an odd t gives rows that start on 2-byte boundaries only.
CASES = [
    (1, 16, 3, 1, (1, 1, 1), "bias_relu", 0.0), (2, 48, 3, 2, (1, 1, 7), "bias", 1.0),
    (3, 64, 3, 1, (1, 9, 11), "bias_relu", 1.0), (4, 80, 1, 1, (2, 5, 1), "none", 0.0),
    (5, 160, 3, 2, (1, 9, 11), "bias", 0.0), (6, 16, 3, 4, (1, 3, 3), "bias_relu", 1.0),
    (7, 64, 3, 3, (1, 17, 35), "none", 0.0), (8, 48, 3, 2, (2, 8, 33), "bias_relu", 1.0),
    (3, 64, 3, 1, (1, 16, 65), "bias", 0.0),
    (16, 1, 1, 1, (1, 1, 1), "bias", 0.0), (64, 1, 1, 1, (1, 16, 65), "none", 1.0),
    (48, 2, 3, 2, (1, 3, 3), "bias_relu", 0.0), (80, 3, 3, 1, (1, 9, 11), "bias_relu", 1.0),
    (160, 4, 3, 4, (1, 3, 3), "bias", 0.0), (64, 5, 3, 3, (1, 9, 11), "none", 1.0),
    (16, 6, 3, 1, (2, 8, 33), "bias_relu", 0.0), (48, 7, 1, 1, (2, 5, 1), "bias", 1.0),
    (80, 8, 3, 2, (1, 17, 35), "bias_relu", 0.0)]
# what cannet::conv2d_thin_nhwc refuses: ci, co, k, dilation, fp32_out, x dtype
REFUSALS = [
    (3, 4, 3, 1, False, torch.bfloat16), (16, 16, 3, 1, False, torch.bfloat16), (12, 64, 3, 1, False, torch.bfloat16),
    (64, 9, 1, 1, False, torch.bfloat16), (3, 24, 3, 1, False, torch.bfloat16), (3, 64, 5, 1, False, torch.bfloat16),
    (3, 64, 3, 0, False, torch.bfloat16), (64, 1, 3, 5, False, torch.bfloat16), (3, 64, 3, 1, True, torch.bfloat16),
    (3, 64, 3, 1, False, torch.float32)]


def _conv():
    from can_distributed_pytorch_amd.ops import conv as C
    return C


def _refused(device):
    for ci, co, k, dil, f32, dt in REFUSALS:
        with pytest.raises(ValueError):
            torch.ops.cannet.conv2d_thin_nhwc(torch.empty(1, 8, 8, ci, dtype=dt, device=device),
                                              torch.empty(co, ci, k, k, device=device), None, dil, True, f32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci,co,k,dil,nhw,epi,beta", CASES)
def test_forward_and_dgrad_exact(ci, co, k, dil, nhw, epi, beta, dtype):
    C = _conv()
    x16, x = R.int_operand((*nhw, ci), R.X_FIRST if ci <= 8 else R.X_ACT, dtype, 1, DEV)
    w16, w = R.int_operand((co, ci, k, k), R.W_FWD, dtype, 2, DEV)
    b32, b = R.int_operand((co,), R.B_FWD, torch.float32, 3, DEV)
    dy16, dy = R.int_operand((*nhw, co), R.X_ACT, dtype, 4, DEV)
    shift = R.W_FWD[2]
    assert R.exactness_bound(lambda a, c, d: R.conv_fwd_ref(a, c, d, dil, "bias"), (x, w, b), shift) < R.LIMIT
    assert R.exactness_bound(lambda a, c: R.dgrad_ref(a, c, dil), (dy, w), shift) < R.LIMIT
    code = {"bias_relu": C.EPI_BIAS_RELU, "bias": C.EPI_BIAS, "none": C.EPI_NONE}[epi]
    bias = None if epi == "none" else b32
    y = C.conv_thin(x16, C.pack_weight_fwd(w16.float(), dtype), bias, ksize=k, dil=dil, epi=code)
    dx = C.conv_thin(dy16, C.pack_weight_dgrad(w16.float(), dtype), None, ksize=k, dil=dil, epi=C.EPI_NONE)
    ref = R.conv_fwd_ref(x, w, b, dil, epi)
    assert torch.equal(y, R.to16(ref, dtype))
    assert torch.equal(dx, R.to16(R.dgrad_ref(dy, w, dil), dtype))
    if co <= 8:
        y32 = C.conv_thin(x16, C.pack_weight_fwd(w16.float(), dtype), bias, ksize=k, dil=dil, epi=code, fp32_out=True)
        assert y32.dtype == torch.float32 and torch.equal(y32, R.to32(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci,co,k,dil,nhw,epi,beta", CASES)
def test_wgrad_exact(ci, co, k, dil, nhw, epi, beta, dtype):
    C = _conv()
    x16, x = R.int_operand((*nhw, ci), R.X_WG, dtype, 5, DEV)
    dy16, dy = R.int_operand((*nhw, co), R.X_WG, dtype, 6, DEV)
    dw, dw0 = R.int_operand((co, ci, k, k), R.X_ACT, torch.float32, 7, DEV)
    db, db0 = R.int_operand((co,), R.X_ACT, torch.float32, 8, DEV)
    assert R.exactness_bound(lambda a, c: R.wgrad_ref(a, c, k, dil), (dy, x), 0) * 2 + 12 < R.LIMIT     # scale 2, |dw0| <= 12
    C.conv_thin_wgrad(dy16, x16, dw, db if epi != "none" else None, ksize=k, dil=dil, beta=beta, scale=2.0)
    rw, rb = R.wgrad_ref(dy, x, k, dil)
    assert torch.equal(dw, R.to32(R.wgrad_update_ref(rw, dw0, beta, 2.0)))
    assert torch.equal(db, R.to32(R.wgrad_update_ref(rb, db0, beta, 2.0) if epi != "none" else db0))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci,co,k,dil,relu,f32,xgrad", [(3, 64, 3, 1, True, False, True), (64, 1, 1, 1, False, True, True),
                                                        (48, 4, 3, 2, True, False, True), (3, 64, 3, 1, True, False, False)])
def test_conv2d_thin_nhwc_vs_aten(ci, co, k, dil, relu, f32, xgrad, dtype):
    rel = lambda a, b: ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()  # noqa: E731
    torch.manual_seed(0)
    x = torch.randn(2, 19, 37, ci, device=DEV).to(dtype)
    m = L.Conv2dThinNHWC(ci, co, k, dilation=dil, relu=relu, fp32_out=f32).cuda()
    with torch.no_grad():
        m.weight.normal_(0, 0.05)
        m.bias.normal_(0, 0.1)
        m.weight.copy_(m.weight.to(dtype).float())               # the reference sees the 16-bit-rounded weights
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wr, br = m.weight.detach().clone().requires_grad_(True), m.bias.detach().clone().requires_grad_(True)
    z = F.conv2d(xr, wr, br, padding=dil * (k // 2), dilation=dil)
    xg = x.clone().requires_grad_(xgrad)
    y = m(xg)
    assert y.dtype == (torch.float32 if f32 else dtype) and y.shape == (2, 19, 37, co)
    assert rel(y.float().permute(0, 3, 1, 2), F.relu(z) if relu else z) < 1e-2
    g = torch.randn_like(z)
    y.backward(g.permute(0, 2, 3, 1).to(y.dtype))
    dz = g.to(dtype).float()
    if relu:
        dz = dz * (y.float().permute(0, 3, 1, 2) > 0)            # the op's own ReLU mask, as test_library_ops
    refs = torch.autograd.grad(z, [xr, wr, br], dz)
    if xgrad:
        assert rel(xg.grad.float().permute(0, 3, 1, 2), refs[0]) < 1e-2
    else:
        assert xg.grad is None                                   # an image: no data gradient is computed
    assert rel(m.weight.grad, refs[1]) < 1e-2
    assert rel(m.bias.grad, refs[2]) < 1e-2


@pytest.mark.gpu
def test_opcheck_and_compile_thin():
    x = torch.randn(1, 8, 19, 3, device=DEV).to(torch.bfloat16)
    w, b = torch.randn(64, 3, 3, 3, device=DEV) * 0.05, torch.randn(64, device=DEV)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.cannet.conv2d_thin_nhwc.default, (x, w, b, 1, True, False), test_utils=utils)
    xh = torch.randn(1, 8, 19, 64, device=DEV).to(torch.bfloat16)
    torch.library.opcheck(torch.ops.cannet.conv2d_thin_nhwc.default,
                          (xh, torch.randn(2, 64, 1, 1, device=DEV), None, 1, False, True), test_utils=utils)
    m = torch.nn.Sequential(L.Conv2dThinNHWC(3, 64, 3), L.Conv2dNHWC(64, 64),
                            L.Conv2dThinNHWC(64, 1, 1, relu=False, fp32_out=True)).cuda()
    assert torch.equal(torch.compile(m, fullgraph=True, backend="aot_eager")(x), m(x))


@pytest.mark.gpu
def test_wgrad_repeatable_and_refusals():
    C = _conv()
    torch.manual_seed(0)
    for ci, co in ((3, 64), (64, 4)):
        x = torch.randn(2, 40, 70, ci, device=DEV).to(torch.bfloat16)
        dy = torch.randn(2, 40, 70, co, device=DEV).to(torch.bfloat16)
        assert C.conv_thin_ws_floats(2 * 40 * 70, ci, co, 3) >= 8 * (ci * co * 9 + co)      # several slices
        outs = []
        for _ in range(2):
            dw, db = torch.empty(co, ci, 3, 3, device=DEV), torch.empty(co, device=DEV)
            C.conv_thin_wgrad(dy, x, dw, db, ksize=3, dil=2)
            outs.append((dw, db))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    _refused(DEV)


def test_thin_shapes_and_refusals_cpu():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 24, 31, 3, dtype=torch.float16)
        y = torch.ops.cannet.conv2d_thin_nhwc(x, torch.empty(64, 3, 3, 3), torch.empty(64), 1, True, False)
        assert y.shape == (2, 24, 31, 64) and y.dtype == torch.float16
        y = torch.ops.cannet.conv2d_thin_nhwc(y, torch.empty(4, 64, 1, 1), None, 1, False, True)
        assert y.shape == (2, 24, 31, 4) and y.dtype == torch.float32
        _refused("cpu")
