"""torch.ops.cannet.group_norm_nhwc / GroupNorm2dNHWC / InstanceNorm2dNHWC (ops/library.py): registration, fake shapes,
the op's checks and the state dicts on the CPU; on the GPU the op against fp32 ATen, opcheck and torch.compile."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from can_distributed_pytorch_amd.ops import library as L


def test_registered_and_fake_shapes_cpu():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.cannet, "group_norm_nhwc") and hasattr(torch.ops.cannet, "group_norm_nhwc_backward")
    with FakeTensorMode():
        x, v = torch.empty(2, 8, 12, 24, dtype=torch.float16), torch.empty(24)
        y, stats = torch.ops.cannet.group_norm_nhwc(x, v, v, 8, 1e-5, True)
        assert y.shape == x.shape and y.dtype == x.dtype
        assert stats.shape == (2, 8, 3) and stats.dtype == torch.float32
        dx, dg, db = torch.ops.cannet.group_norm_nhwc_backward(y, x, y, v, stats, 8, True)
        assert dx.shape == x.shape and dx.dtype == x.dtype and dg.shape == db.shape == (24,) and dg.dtype == torch.float32
        for bad in ((torch.empty(1, 2, 2, 12, dtype=torch.float16), torch.empty(12), 4),      # C % 8
                    (x, v, 5),                                                                 # C % G
                    (torch.empty(1, 1, 1, 24, dtype=torch.float16), v, 24),                    # one value per group
                    (x.float(), v, 8), (x, v.double(), 8), (x, torch.empty(8), 8)):
            with pytest.raises(ValueError):
                torch.ops.cannet.group_norm_nhwc(bad[0], bad[1], bad[1], bad[2])


@pytest.mark.parametrize("affine", [True, False])
def test_state_dicts_match_torch(affine):
    shapes = lambda mod: {k: (v.shape, v.dtype) for k, v in mod.state_dict().items()}
    for m, ref in ((L.GroupNorm2dNHWC(8, 24, affine=affine), nn.GroupNorm(8, 24, affine=affine)),
                   (L.InstanceNorm2dNHWC(24, affine=affine), nn.InstanceNorm2d(24, affine=affine))):
        assert shapes(m) == shapes(ref) and (len(shapes(m)) == 2) == affine
        assert m.weight.shape == m.bias.shape == (24,)
        if affine:
            with torch.no_grad():
                ref.weight.normal_()
        m.load_state_dict(ref.state_dict())
        ref.load_state_dict(m.state_dict())
        assert not affine or torch.equal(m.weight, ref.weight)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _nchw(t):
    return t.detach().float().permute(0, 3, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,groups", [((2, 8, 12, 32), 4), ((1, 9, 7, 24), 24), ((2, 64, 96, 64), 8)])
def test_op_vs_aten(shape, groups):
    """fp32 ATen on the same 16-bit input, the gradient through the op's own mask; (2, 64, 96, 64) is streamed."""
    torch.manual_seed(0)
    c = shape[-1]
    x = (torch.randn(*shape, device="cuda") * 2 + 1).to(torch.bfloat16).requires_grad_(True)
    w = (torch.rand(c, device="cuda") + 0.5).requires_grad_(True)
    b = torch.randn(c, device="cuda").requires_grad_(True)
    y, _ = torch.ops.cannet.group_norm_nhwc(x, w, b, groups, 1e-5, True)
    g = torch.randn(*shape, device="cuda").to(torch.bfloat16)
    y.backward(g)
    xr, wr, br = _nchw(x).requires_grad_(True), w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    zr = F.group_norm(xr, groups, wr, br, 1e-5)
    assert _rel(_nchw(y), F.relu(zr)) < 1e-2
    refs = torch.autograd.grad(zr * (_nchw(y) > 0), [xr, wr, br], _nchw(g))
    for got, ref in zip((_nchw(x.grad), w.grad, b.grad), refs):
        assert _rel(got, ref) < 1e-2


@pytest.mark.gpu
def test_opcheck():
    x = torch.randn(2, 4, 6, 16, device="cuda").to(torch.bfloat16)
    w, b = torch.rand(16, device="cuda") + 0.5, torch.randn(16, device="cuda")
    y, stats = torch.ops.cannet.group_norm_nhwc(x, w, b, 4, 1e-5, True)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.cannet.group_norm_nhwc.default, (x, w, b, 4, 1e-5, True), test_utils=utils)
    torch.library.opcheck(torch.ops.cannet.group_norm_nhwc_backward.default,
                          (torch.randn_like(x), x, y, w, stats, 4, True), test_utils=utils[:2])


@pytest.mark.gpu
def test_compile_fullgraph():
    torch.manual_seed(0)
    net = nn.Sequential(L.Conv2dNHWC(16, 32, relu=False), L.InstanceNorm2dNHWC(32), L.ReluMaxPool2x2()).cuda()
    x = torch.randn(2, 8, 12, 16, device="cuda").to(torch.bfloat16)
    assert torch.equal(torch.compile(net, fullgraph=True, backend="aot_eager")(x), net(x))
