"""torch.ops.cannet.batch_norm_nhwc / BatchNorm2dNHWC (ops/library.py): registration, fake shapes and state dict on the
CPU; on the GPU the conv -> BN -> pool stack against fp32 ATen, the running buffers, opcheck and torch.compile."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from can_distributed_pytorch_amd.ops import library as L


def test_registered_and_fake_shapes_cpu():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.cannet, "batch_norm_nhwc") and hasattr(torch.ops.cannet, "batch_norm_nhwc_backward")
    with FakeTensorMode():
        x = torch.empty(2, 8, 12, 32, dtype=torch.float16)
        v = torch.empty(32)
        for args in ((x, v, v, None, None, True), (x, v, v, v, v, False)):
            y, stats = torch.ops.cannet.batch_norm_nhwc(*args, 1e-5, True)
            assert y.shape == x.shape and y.dtype == x.dtype
            assert stats.shape == (3, 32) and stats.dtype == torch.float32
        dx, dg, db = torch.ops.cannet.batch_norm_nhwc_backward(y, x, y, v, stats, True, True)
        assert dx.shape == x.shape and dx.dtype == x.dtype and dg.shape == db.shape == (32,) and dg.dtype == torch.float32
        with pytest.raises(ValueError):
            torch.ops.cannet.batch_norm_nhwc(torch.empty(1, 2, 2, 12, dtype=torch.float16), v, v, None, None, True)


def test_state_dict_matches_batchnorm2d():
    m, ref = L.BatchNorm2dNHWC(24), nn.BatchNorm2d(24)
    shapes = lambda mod: {k: (v.shape, v.dtype) for k, v in mod.state_dict().items()}
    assert shapes(m) == shapes(ref)
    with torch.no_grad():
        ref.running_mean.normal_()
        ref.num_batches_tracked += 3
    m.load_state_dict(ref.state_dict())
    ref.load_state_dict(m.state_dict())
    assert torch.equal(m.running_mean, ref.running_mean) and int(m.num_batches_tracked) == 3


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _stack():
    torch.manual_seed(0)
    net = nn.Sequential(L.Conv2dNHWC(16, 32, relu=False), L.BatchNorm2dNHWC(32), L.ReluMaxPool2x2()).cuda()
    with torch.no_grad():
        net[0].weight.normal_(0, 0.1)
        net[0].bias.normal_(0, 0.5)
        net[1].weight.normal_(1, 0.3)
        net[1].bias.normal_(0, 0.3)
    return net, torch.randn(2, 8, 12, 16, device="cuda").to(torch.bfloat16)


def _nchw(t):
    return t.detach().float().permute(0, 3, 1, 2)


@pytest.mark.gpu
def test_stack_vs_aten():
    """fp32 ATen of the same stack, stage by stage, every stage fed the op's own 16-bit upstream tensor (forward) and
    downstream gradient (backward): a 16-bit rounding upstream can flip a ReLU sign or a pool argmax, which moves whole
    gradient entries and is no error of the stage that follows."""
    net, x = _stack()
    bn = nn.BatchNorm2d(32).cuda()
    bn.load_state_dict(net[1].state_dict())
    xg = x.clone().requires_grad_(True)
    z = net[0](xg)
    yb = net[1](z)
    y = net[2](yb)
    z.retain_grad()
    yb.retain_grad()
    g = torch.randn(2, 4, 6, 32, device="cuda").to(torch.bfloat16)
    y.backward(g)
    xr, zin, pin = (_nchw(t).requires_grad_(True) for t in (x, z, yb))
    zr, br, pr = F.conv2d(xr, net[0].weight, net[0].bias, padding=1), bn(zin), F.max_pool2d(F.relu(pin), 2)
    assert _rel(_nchw(z), zr) < 1e-2 and _rel(_nchw(yb), F.relu(br)) < 1e-2 and torch.equal(_nchw(y), pr)
    (dpin,) = torch.autograd.grad(pr, pin, _nchw(g))
    dbn = torch.autograd.grad(br * (_nchw(yb) > 0), [zin, bn.weight, bn.bias], _nchw(yb.grad))
    dconv = torch.autograd.grad(zr, [xr, net[0].weight, net[0].bias], _nchw(z.grad))
    got = [_nchw(yb.grad), _nchw(z.grad), net[1].weight.grad, net[1].bias.grad, _nchw(xg.grad), net[0].weight.grad,
           net[0].bias.grad]
    for a, b in zip(got, (dpin,) + dbn + dconv):
        assert _rel(a, b) < 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("momentum", [0.1, None])
def test_running_buffers_and_eval(momentum):
    net, x = _stack()
    net[1].momentum = momentum
    bn = nn.BatchNorm2d(32, momentum=momentum).cuda()
    bn.load_state_dict(net[1].state_dict())
    with torch.no_grad():
        for i in range(2):
            xi = x if i == 0 else (x.float() * 0.5 + 0.25).to(torch.bfloat16)
            z = net[0](xi)                        # nn.BatchNorm2d is fed the same conv output
            net[1](z)
            bn(z.float().permute(0, 3, 1, 2))
        assert int(net[1].num_batches_tracked) == int(bn.num_batches_tracked) == 2
        # the statistics are double sums of the same 16-bit values on both sides up to ATen's fp32 accumulation
        assert torch.allclose(net[1].running_mean, bn.running_mean, rtol=1e-5, atol=1e-6)
        assert torch.allclose(net[1].running_var, bn.running_var, rtol=1e-5, atol=1e-6)
        net.eval()
        bn.eval()
        z, before = net[0](x), net[1].running_mean.clone()
        y = net[1](z)
        assert _rel(y.float().permute(0, 3, 1, 2), F.relu(bn(z.float().permute(0, 3, 1, 2)))) < 1e-2
        assert torch.equal(net[1].running_mean, before) and int(net[1].num_batches_tracked) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("training", [True, False])
def test_opcheck(training):
    x = torch.randn(1, 4, 6, 16, device="cuda").to(torch.bfloat16)
    w, b = torch.rand(16, device="cuda") + 0.5, torch.randn(16, device="cuda")
    rm, rv = torch.randn(16, device="cuda"), torch.rand(16, device="cuda") + 0.5
    y, stats = torch.ops.cannet.batch_norm_nhwc(x, w, b, rm, rv, training, 1e-5, True)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.cannet.batch_norm_nhwc.default, (x, w, b, rm, rv, training, 1e-5, True),
                          test_utils=utils)
    torch.library.opcheck(torch.ops.cannet.batch_norm_nhwc_backward.default,
                          (torch.randn_like(x), x, y, w, stats, training, True), test_utils=utils[:2])


@pytest.mark.gpu
def test_compile_fullgraph():
    net, x = _stack()
    ref = net(x)
    mean1 = net[1].running_mean.clone()
    with torch.no_grad():
        net[1].running_mean.zero_()
        net[1].running_var.fill_(1)
        net[1].num_batches_tracked.zero_()
    out = torch.compile(net, fullgraph=True, backend="aot_eager")(x)
    assert torch.equal(out, ref) and torch.equal(net[1].running_mean, mean1)
