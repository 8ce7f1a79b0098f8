"""Large-kernel convolutions (csrc/conv_large.hip; 5x5 at dilation 1 - 2 and 7x7 at dilation 1, Ci and Co any multiples
of 16): bit for bit against the fp64 references of tests/conv_exact_reference.py with the exactly representable operands
of tests/test_gpu_conv_exact.py (asserted bound < 2^24, ``torch.equal``, no tolerance), through the public op against
fp32 ATen with the thresholds of tests/test_library_ops.py, the weight gradient's repeatability, and the refusals."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_reference as R
from can_distributed_pytorch_amd.ops import library as L

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
# ci, co, k, dil, (n, h, w), forward epilogue, beta of the weight gradient
CASES = [
    (16, 16, 5, 1, (1, 1, 1), "bias_relu", 0.0),      # one-pixel map
    (16, 16, 7, 1, (1, 1, 5), "bias", 1.0),           # map narrower than the kernel
    (48, 32, 5, 2, (2, 5, 1), "none", 0.0),           # one column, 16-channel tail, dilation 2
    (32, 48, 7, 1, (1, 9, 33), "bias_relu", 1.0),     # one row and one column past a tile
    (80, 96, 5, 1, (1, 17, 35), "bias", 0.0),         # three chunks with tail, two passes
    (64, 64, 7, 1, (1, 8, 32), "bias_relu", 0.0),     # both multiples of 64 (the routing), exactly one tile
    (160, 16, 5, 2, (2, 8, 32), "none", 1.0),
    (16, 80, 7, 1, (3, 9, 11), "bias_relu", 1.0),     # a pass of four blocks plus an odd single block
    (128, 64, 5, 1, (1, 16, 65), "bias", 0.0)]        # several weight-gradient slices


def _conv():
    from can_distributed_pytorch_amd.ops import conv as C
    return C


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci,co,k,dil,nhw,epi,beta", CASES)
def test_forward_and_dgrad_exact(ci, co, k, dil, nhw, epi, beta, dtype):
    C = _conv()
    x16, x = R.int_operand((*nhw, ci), R.X_ACT, dtype, 1, DEV)
    w16, w = R.int_operand((co, ci, k, k), R.W_FWD, dtype, 2, DEV)
    b32, b = R.int_operand((co,), R.B_FWD, torch.float32, 3, DEV)
    dy16, dy = R.int_operand((*nhw, co), R.X_ACT, dtype, 4, DEV)
    shift = R.W_FWD[2]
    assert R.exactness_bound(lambda a, c, d: R.conv_fwd_ref(a, c, d, dil, "bias"), (x, w, b), shift) < R.LIMIT
    assert R.exactness_bound(lambda a, c: R.dgrad_ref(a, c, dil), (dy, w), shift) < R.LIMIT
    code = {"bias_relu": C.EPI_BIAS_RELU, "bias": C.EPI_BIAS, "none": C.EPI_NONE}[epi]
    y = C.conv_small(x16, C.pack_weight_fwd(w16.float(), dtype), None if epi == "none" else b32, ksize=k, dil=dil,
                     epi=code)
    dx = C.conv_small(dy16, C.pack_weight_dgrad(w16.float(), dtype), None, ksize=k, dil=dil, epi=C.EPI_NONE)
    torch.cuda.synchronize()
    assert torch.equal(y, R.to16(R.conv_fwd_ref(x, w, b, dil, epi), dtype))
    assert torch.equal(dx, R.to16(R.dgrad_ref(dy, w, dil), dtype))


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
    C.conv_small_wgrad(dy16, x16, dw, db if epi != "none" else None, ksize=k, dil=dil, beta=beta, scale=2.0)
    torch.cuda.synchronize()
    rw, rb = R.wgrad_ref(dy, x, k, dil)
    assert torch.equal(dw, R.to32(R.wgrad_update_ref(rw, dw0, beta, 2.0)))
    assert torch.equal(db, R.to32(R.wgrad_update_ref(rb, db0, beta, 2.0) if epi != "none" else db0))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci,co,k,dil", [(32, 48, 5, 2), (64, 64, 7, 1)])
def test_conv2d_nhwc_large_vs_aten(ci, co, k, dil, dtype):
    rel = lambda a, b: ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()  # noqa: E731
    torch.manual_seed(0)
    x = torch.randn(2, 19, 37, ci, device=DEV).to(dtype)
    m = L.Conv2dNHWC(ci, co, k, dilation=dil).cuda()
    with torch.no_grad():
        m.weight.normal_(0, 0.05)
        m.bias.normal_(0, 0.1)
        m.weight.copy_(m.weight.to(dtype).float())               # the reference sees the 16-bit-rounded weights
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wr, br = m.weight.detach().clone().requires_grad_(True), m.bias.detach().clone().requires_grad_(True)
    z = F.conv2d(xr, wr, br, padding=dil * (k // 2), dilation=dil)
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    assert y.dtype == dtype and y.shape == (2, 19, 37, co)
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
    x = torch.randn(2, 40, 70, 48, device=DEV).to(torch.bfloat16)
    dy = torch.randn(2, 40, 70, 32, device=DEV).to(torch.bfloat16)
    assert C.conv_small_ws_floats(2 * 40 * 70, 48, 32, 5) > 48 * 32 * 25 + 32         # several slices
    outs = []
    for _ in range(2):
        dw, db = torch.empty(32, 48, 5, 5, device=DEV), torch.empty(32, device=DEV)
        C.conv_small_wgrad(dy, x, dw, db, ksize=5, dil=1)
        outs.append((dw, db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.gpu
def test_opcheck_and_compile_large():
    x = torch.randn(1, 8, 16, 32, device=DEV).to(torch.bfloat16)
    w, b = torch.randn(48, 32, 7, 7, device=DEV) * 0.05, torch.randn(48, device=DEV)
    torch.library.opcheck(torch.ops.cannet.conv2d_nhwc.default, (x, w, b, 1, True),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    m = torch.nn.Sequential(L.Conv2dNHWC(32, 48, 7), L.Conv2dNHWC(48, 16, 5, dilation=2)).cuda()
    assert torch.equal(torch.compile(m, fullgraph=True, backend="aot_eager")(x), m(x))


def test_large_kernel_shapes_cpu():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 24, 32, 32, dtype=torch.bfloat16)
        y = torch.ops.cannet.conv2d_nhwc(x, torch.empty(48, 32, 5, 5), torch.empty(48), 2, True)
        assert y.shape == (2, 24, 32, 48) and y.dtype == torch.bfloat16
        for k, dil in [(9, 1), (4, 1), (7, 2), (5, 3)]:
            with pytest.raises(ValueError):
                torch.ops.cannet.conv2d_nhwc(x, torch.empty(48, 32, k, k), torch.empty(48), dil, True)
