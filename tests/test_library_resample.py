"""torch.ops.cannet.adaptive_avg_pool_nhwc / resize_bilinear_nhwc and their modules (ops/library.py): registration, fake
shapes and the modules' size arithmetic on the CPU; on the GPU opcheck, torch.compile and one CANNet context branch
built from library modules only against fp32 ATen."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from can_distributed_pytorch_amd.ops import library as L


def test_registered_and_fake_shapes_cpu():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("adaptive_avg_pool_nhwc", "resize_bilinear_nhwc"):
        assert hasattr(torch.ops.cannet, name) and hasattr(torch.ops.cannet, name + "_backward")
    with FakeTensorMode():
        for dtype in (torch.float16, torch.bfloat16):
            x = torch.empty(2, 5, 7, 24, dtype=dtype)
            y = torch.ops.cannet.adaptive_avg_pool_nhwc(x, 3, 9)
            z = torch.ops.cannet.resize_bilinear_nhwc(x, 11, 4, True)
            assert y.shape == (2, 3, 9, 24) and z.shape == (2, 11, 4, 24) and y.dtype == z.dtype == dtype
            dx = torch.ops.cannet.adaptive_avg_pool_nhwc_backward(y, 5, 7)
            dz = torch.ops.cannet.resize_bilinear_nhwc_backward(z, 5, 7, True)
            assert dx.shape == dz.shape == x.shape and dx.dtype == dz.dtype == dtype
        for bad in (torch.empty(1, 2, 2, 12, dtype=torch.float16), torch.empty(1, 2, 2, 8)):
            with pytest.raises(ValueError):
                torch.ops.cannet.resize_bilinear_nhwc(bad, 4, 4, False)


@pytest.mark.parametrize("kw", [dict(size=9), dict(size=(4, 11)), dict(scale_factor=2), dict(scale_factor=1.5),
                                dict(scale_factor=(0.5, 2.6))])
def test_module_sizes_match_interpolate(kw):
    m = L.ResizeBilinearNHWC(**kw)
    for h, w in ((7, 5), (12, 20)):
        ref = F.interpolate(torch.zeros(1, 1, h, w), mode="bilinear", **kw)
        assert m.output_size(h, w) == tuple(ref.shape[2:])
    assert L.AdaptiveAvgPool2dNHWC(3).output_size == (3, 3) and L.AdaptiveAvgPool2dNHWC((2, 5)).output_size == (2, 5)
    with pytest.raises(ValueError):
        L.ResizeBilinearNHWC()


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _nchw(t):
    return t.detach().float().permute(0, 3, 1, 2)


def _branch(s=3, hw=(12, 20)):
    torch.manual_seed(0)
    net = nn.Sequential(L.AdaptiveAvgPool2dNHWC(s), L.Conv2dNHWC(64, 64, kernel_size=1, bias=False, relu=False),
                        L.ResizeBilinearNHWC(size=hw, align_corners=True)).cuda()
    with torch.no_grad():
        net[1].weight.normal_(0, 0.1)
    return net, torch.randn(2, *hw, 64, device="cuda").to(torch.bfloat16)


@pytest.mark.gpu
def test_context_branch_vs_aten():
    """CANNet's context branch (model/CANNet.py: adaptive_avg_pool2d -> 1x1 conv -> bilinear upsample) in fp32 ATen
    on the same 16-bit operands; tolerance: tests/test_library_batchnorm.py's for its conv -> BN -> pool stack."""
    net, x = _branch()
    xg = x.clone().requires_grad_(True)
    y = net(xg)
    g = torch.randn_like(y)
    y.backward(g)
    xr = _nchw(x).requires_grad_(True)
    yr = F.interpolate(F.conv2d(F.adaptive_avg_pool2d(xr, 3), net[1].weight), size=(12, 20), mode="bilinear",
                       align_corners=True)
    dxr, dwr = torch.autograd.grad(yr, [xr, net[1].weight], _nchw(g))
    assert y.shape == x.shape and y.dtype == x.dtype
    assert _rel(_nchw(y), yr) < 1e-2 and _rel(_nchw(xg.grad), dxr) < 1e-2 and _rel(net[1].weight.grad, dwr) < 1e-2


@pytest.mark.gpu
def test_opcheck():
    x = torch.randn(1, 5, 6, 16, device="cuda").to(torch.bfloat16)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.cannet.adaptive_avg_pool_nhwc.default, (x, 2, 4), test_utils=utils)
    torch.library.opcheck(torch.ops.cannet.resize_bilinear_nhwc.default, (x, 9, 4, False), test_utils=utils)
    torch.library.opcheck(torch.ops.cannet.adaptive_avg_pool_nhwc_backward.default, (x, 7, 3), test_utils=utils[:2])
    torch.library.opcheck(torch.ops.cannet.resize_bilinear_nhwc_backward.default, (x, 7, 3, True), test_utils=utils[:2])


@pytest.mark.gpu
def test_compile_fullgraph():
    net, x = _branch()
    ref = net(x)
    out = torch.compile(net, fullgraph=True, backend="aot_eager")(x)
    assert torch.equal(out, ref)
