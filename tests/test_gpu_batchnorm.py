"""csrc/batchnorm.hip (ops/batchnorm.py) against plain fp64: ATen's batch_norm on x.double() in NCHW, then relu, gradients by
fp64 autograd through the kernel's own mask y > 0.  Bit for bit on exactly representable operands, and against bounds
derived from the kernels' rounding steps on random ones (README, "Batch normalisation")."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]


def _ref(x, gamma, beta, rm, rv, training, eps, dy=None, ymask=None):
    """fp64 (pre-ReLU output, mean, biased var) and, with dy, (dx, dgamma, dbeta) through the mask ymask (or none)."""
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    # the ATen call behind F.batch_norm, which itself refuses the exact tests' eps = 0
    z = torch.batch_norm(x64.permute(0, 3, 1, 2), g64, b64, None if training else rm.double(), None if training else rv.double(),
                         training, 0.0, eps, False).permute(0, 2, 3, 1)
    mean = x64.detach().mean((0, 1, 2)) if training else rm.double()
    var = x64.detach().var((0, 1, 2), unbiased=False) if training else rv.double()
    grads = None
    if dy is not None:
        out = z if ymask is None else z * ymask
        grads = torch.autograd.grad(out, [x64, g64, b64], dy.double())
    return z.detach(), mean, var, grads


def _exact_case(n, h, w, c, dtype):
    """x = (k +- 1) s per channel in equal counts, s a power of two: mean = k s, var = s^2, rstd = 1 / s are exact, and so
    is every product below (gamma, beta in quarters, dy in eighths; eval: running stats with 1 / sqrt(rv) = 2^-j / s)."""
    g = torch.Generator().manual_seed(n * 1000 + h * 100 + w * 10 + c)
    m = n * h * w
    s = 2.0 ** torch.randint(-2, 3, (c,), generator=g).double()
    k = torch.randint(-15, 16, (c,), generator=g).double()
    sign = torch.ones(m, c, dtype=torch.float64)
    sign[m // 2:] = -1
    sign = sign.gather(0, torch.rand(m, c, generator=g).argsort(0))
    x = ((k + sign) * s).reshape(n, h, w, c)
    gamma = torch.randint(-7, 8, (c,), generator=g).double() / 4
    gamma[::5] = 0
    beta = torch.randint(-7, 8, (c,), generator=g).double() / 4
    dy = (torch.randint(-7, 8, (m, c), generator=g).double() / 8).reshape(n, h, w, c)
    rm = torch.randint(-15, 16, (c,), generator=g).double() * s
    rv = (s * 2.0 ** torch.randint(-1, 2, (c,), generator=g).double()) ** 2
    # exactness bound (fp32 holds integers below 2^24).  Training, in units of 1 / (8 M): |dz - c1 - xhat c2| <= 21 M,
    # times |gamma| in quarters <= 7.  Eval, in sixteenths: |sum dz xhat| <= M * 7 * 62 (|xhat| <= 31 * 2).
    assert max(7 * 21 * m, m * 7 * 62) < 2 ** 24
    return x.to(dtype), gamma.float(), beta.float(), rm.float(), rv.float(), dy.to(dtype)


EXACT = [(1, 1, 2, 8, 0), (1, 3, 6, 24, 1), (2, 8, 16, 64, 3), (1, 16, 16, 136, 7), (4, 16, 64, 264, 0),
         (2, 8, 16, 8, 5)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("n,h,w,c,slices", EXACT)
def test_bit_for_bit(n, h, w, c, slices, relu, training, dtype):
    from can_distributed_pytorch_amd.ops import batchnorm as BN
    host = _exact_case(n, h, w, c, dtype)
    x, gamma, beta, rm, rv, dy = (t.cuda() for t in host)
    y, stats = BN.bn_forward(x, gamma, beta, rm, rv, training, 0.0, relu, slices=slices)
    m = n * h * w
    backward = m & (m - 1) == 0                       # c1, c2 are exact for a power-of-two pixel count only
    # the reference runs on the host, where ATen's fp64 batch norm takes plain sums (exact here), not Welford updates
    z, mean, var, grads = _ref(*host[:5], training, 0.0, host[5] if backward else None,
                               (y > 0).cpu() if relu else None)
    assert torch.equal(y.cpu(), (z.relu() if relu else z).to(dtype))
    assert torch.equal(stats.cpu(), torch.stack([mean, var, 1 / var.sqrt()]).float())
    if backward:
        dx, dg, db = BN.bn_backward(dy, x, y, gamma, stats, training, relu, slices=slices)
        assert torch.equal(dx.cpu(), grads[0].to(dtype))
        assert torch.equal(dg.cpu(), grads[1].float()) and torch.equal(db.cpu(), grads[2].float())


RANDOM = [(1, 5, 7, 8), (3, 9, 11, 24), (2, 37, 61, 136), (1, 17, 35, 264)]


def _ratio(name, got, ref, bound):
    r = ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"err/bound {name}: {r:.3f}")
    return r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slices", [0, 2])
@pytest.mark.parametrize("n,h,w,c", RANDOM)
def test_random_against_fp64(n, h, w, c, slices, dtype):
    """Bounds.  half(v) = half an ulp of the one 16-bit rounding of v: u |v| with u = 2^-8 (bf16) / 2^-11 (fp16), and
    the format's fixed spacing below its smallest normal number, 2^-25 for fp16 (2^-134 for bf16) -- with u |v| alone the
    fp16 dx of (3, 9, 11, 24) measured err / bound = 3.9 on an output of 1e-6, where fp16 values are 2^-24 apart.
    e = 2^-24 per fp32 rounding on the kernel's path:
    y:      5 roundings (mean, rstd, a = gamma rstd, b = fma(-mean, a, beta), fma(x, a, b)), each relative to a term of
            |x a| + |mean a| + |beta|.
    dx:     10 (mean, rstd, a, x - mean, (.) rstd, c1, c2, dz - c1, fma(-xhat, c2, .), a (.)) over |a| (|dz| + |c1| +
            |xhat c2|) plus the cancellation in x - mean, |a c2| |mean| rstd.
    dgamma: 5 (the four of xhat, the final fp32 rounding of the double sum) over sum |dz xhat| + sum |dz| |mean| rstd;
    dbeta:  1 (the double sum is exact to 2^-53) over sum |dz|."""
    from can_distributed_pytorch_amd.ops import batchnorm as BN
    torch.manual_seed(c + slices)
    u, e, eps = (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11), 2.0 ** -24, 1e-5
    half = lambda v: (u * v.abs()).clamp_min(2.0 ** (-134 if dtype == torch.bfloat16 else -25))
    spread = torch.rand(c, device="cuda") + 0.25
    x = torch.randn(n, h, w, c, device="cuda") * spread + 8 * spread * (2 * torch.rand(c, device="cuda") - 1)
    x[..., 3] = 1.75                                   # a constant channel: var = 0, rstd = 1 / sqrt(eps)
    x = x.to(dtype)
    gamma, beta = torch.randn(c, device="cuda"), torch.randn(c, device="cuda")
    dy = torch.randn(n, h, w, c, device="cuda").to(dtype)
    y, stats = BN.bn_forward(x, gamma, beta, None, None, True, eps, True, slices=slices)
    dx, dg, db = BN.bn_backward(dy, x, y, gamma, stats, True, True, slices=slices)
    y2, stats2 = BN.bn_forward(x, gamma, beta, None, None, True, eps, True, slices=slices)
    again = BN.bn_backward(dy, x, y, gamma, stats, True, True, slices=slices)
    assert torch.equal(y, y2) and torch.equal(stats, stats2)
    assert all(torch.equal(p, q) for p, q in zip((dx, dg, db), again))
    z, mean, var, grads = _ref(x, gamma, beta, None, None, True, eps, dy, y > 0)
    rstd = 1 / (var + eps).sqrt()
    a, x64 = gamma.double() * rstd, x.double()
    r = [_ratio("y", y, z.relu(), half(z.relu()) + 5 * e * ((x64 * a).abs() + (mean * a).abs() + beta.abs()))]
    dz = dy.double() * (y > 0)
    xhat = (x64 - mean) * rstd
    m = n * h * w
    c1, c2 = dz.sum((0, 1, 2)) / m, (dz * xhat).sum((0, 1, 2)) / m
    mag = a.abs() * (dz.abs() + c1.abs() + (xhat * c2).abs()) + (a * c2).abs() * mean.abs() * rstd
    r.append(_ratio("dx", dx, grads[0], half(grads[0]) + 10 * e * mag))
    sums = (dz * xhat).abs().sum((0, 1, 2)) + dz.abs().sum((0, 1, 2)) * mean.abs() * rstd
    r.append(_ratio("dgamma", dg, grads[1], 5 * e * sums))
    r.append(_ratio("dbeta", db, grads[2], e * dz.abs().sum((0, 1, 2))))
    assert max(r) <= 1.0, r


def test_refusals():
    from can_distributed_pytorch_amd.ops import _ext, batchnorm as BN
    v = lambda c: torch.ones(c, device="cuda")
    x = lambda *s, d=torch.bfloat16: torch.zeros(*s, device="cuda", dtype=d)
    for args in ((x(1, 2, 2, 12), v(12), v(12), None, None, True, 1e-5, True),        # C % 8
                 (x(1, 1, 1, 8), v(8), v(8), None, None, True, 1e-5, True),           # one value per channel
                 (x(1, 2, 2, 8), v(8), v(8), None, None, True, -1e-5, True),          # eps < 0
                 (x(1, 2, 2, 8, d=torch.float32), v(8), v(8), None, None, True, 1e-5, True)):
        with pytest.raises(ValueError):
            BN.bn_forward(*args)
    t, raw = x(1, 2, 2, 16), _ext.require().bn_forward
    p = [t.data_ptr()] * 7
    for m, c, eps, dt, rc in ((4, 12, 1e-5, 0, -2), (1, 8, 1e-5, 0, -3), (4, 8, -1.0, 0, -4), (4, 8, float("nan"), 0, -4),
                              (4, 8, 1e-5, 2, -20), (1 << 46, 8, 1e-5, 0, -5)):
        with pytest.raises(RuntimeError, match=f"rc={rc}"):
            raw(*p, 1, t.data_ptr(), t.data_ptr(), m, c, eps, 1, 1, dt, 0)
