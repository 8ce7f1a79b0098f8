"""csrc/groupnorm.hip (ops/groupnorm.py) against plain fp64: F.group_norm on x.double() in NCHW, then relu, gradients by
fp64 autograd through the kernel's own mask y > 0.  Bit for bit on exactly representable operands, and against bounds
derived from the kernels' rounding steps on random ones (README, "Group / instance normalisation"), in every form that
serves the shape."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]


def _ref(x, gamma, beta, groups, eps, dy=None, ymask=None):
    """fp64 (pre-ReLU output, stats [N,G,3]) and, with dy, (dx, dgamma, dbeta) through the mask ymask (or none)."""
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.group_norm(x64.permute(0, 3, 1, 2), groups, g64, b64, eps).permute(0, 2, 3, 1)
    n, h, w, c = x.shape
    xg = x64.detach().reshape(n, h * w, groups, c // groups).permute(0, 2, 1, 3).reshape(n, groups, -1)
    mean = xg.mean(2)
    var = ((xg - mean[..., None]) ** 2).mean(2)
    grads = None
    if dy is not None:
        grads = torch.autograd.grad(z if ymask is None else z * ymask, [x64, g64, b64], dy.double())
    return z.detach(), torch.stack([mean, var, 1 / (var + eps).sqrt()], 2), grads


def _exact_case(n, h, w, c, groups, dtype):
    """x = (k + d) s per (sample, group), s a power of two, integer deviations d with sum 0 over the group's H W cg
    elements: +-1 in equal counts for an even count (var = s^2), and for an odd count (>= 5) +-2 in equal counts plus
    {3, -3, 1, -1, 0} (sum d^2 = 4 count: var = 4 s^2).  mean = k s, var and rstd are then exact, and so is every
    product below (gamma, beta in quarters with some gamma = 0, dy in eighths)."""
    g = torch.Generator().manual_seed(n * 1000 + h * 100 + w * 10 + c + groups)
    cg, cnt = c // groups, h * w * (c // groups)
    s = 2.0 ** torch.randint(-2, 3, (n, groups, 1), generator=g).double()
    k = torch.randint(-15, 16, (n, groups, 1), generator=g).double()
    half = torch.ones((cnt - (5 if cnt % 2 else 0)) // 2, dtype=torch.float64) * (2 if cnt % 2 else 1)
    d = torch.cat([half, -half] + ([torch.tensor([3.0, -3, 1, -1, 0], dtype=torch.float64)] if cnt % 2 else []))
    d = d.expand(n, groups, cnt).gather(2, torch.rand(n, groups, cnt, generator=g).argsort(2))
    x = ((k + d) * s).reshape(n, groups, h * w, cg).permute(0, 2, 1, 3).reshape(n, h, w, c).contiguous()
    gamma = torch.randint(-7, 8, (c,), generator=g).double() / 4
    gamma[::5] = 0
    beta = torch.randint(-7, 8, (c,), generator=g).double() / 4
    dy = (torch.randint(-7, 8, (n, h, w, c), generator=g).double() / 8)
    # exactness bound (fp32 holds integers below 2^24), backward (even counts: xhat = +-1), in units of 1 / (32 count):
    # |gamma dz - c1 - xhat c2| <= 3 * 49 count
    assert 3 * 49 * cnt < 2 ** 24
    return x.to(dtype), gamma.float(), beta.float(), dy.to(dtype)


# (N, H, W, C, G, a slice count that does not divide H W, backward)
EXACT = [(1, 1, 2, 8, 8, 3, True),           # smallest instance norm
         (2, 4, 4, 8, 2, 3, True),           # groups inside one octet
         (2, 4, 8, 16, 2, 3, True),          # a group equal to one octet
         (3, 5, 7, 24, 8, 3, False),         # cg = 3, groups straddling octets, odd pixel count
         (2, 8, 8, 128, 1, 5, True),         # one group across 16 octets
         (2, 8, 16, 48, 3, 3, False),        # a ragged last bundle; H W cg = 2048 but forward only
         (4, 16, 64, 264, 33, 37, True),     # more than 256 channels (two spans), several samples, chunked slice sums
         (1, 40, 40, 64, 64, 7, True)]       # the forward's tile (100 KiB) is resident, the backward's two are not


def _forms(shape, groups, backward, s2):
    from can_distributed_pytorch_amd.ops import groupnorm as GN
    resident = [(GN.RESIDENT, 0)] if GN.plan(shape, groups, backward)["bundle"] else []
    return [(GN.STREAMED, 1), (GN.STREAMED, s2)] + resident


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("n,h,w,c,groups,s2,bwd", EXACT)
def test_bit_for_bit(n, h, w, c, groups, s2, bwd, relu, dtype):
    from can_distributed_pytorch_amd.ops import groupnorm as GN
    host = _exact_case(n, h, w, c, groups, dtype)
    x, gamma, beta, dy = (t.cuda() for t in host)
    cnt = h * w * c // groups
    backward = bwd and cnt & (cnt - 1) == 0            # c1, c2 are exact for a power-of-two count only
    ref = None
    for form, slices in _forms(x.shape, groups, False, s2):
        y, stats = GN.gn_forward(x, gamma, beta, groups, 0.0, relu, form=form, slices=slices)
        if ref is None:                                # one reference per case, on the host; every form must meet it
            ref = _ref(*host[:3], groups, 0.0, host[3] if backward else None, (y > 0).cpu() if relu else None)
        z, rstats, grads = ref
        # every exact output is a multiple of 1/8 (d gamma [/ 2] + beta).  ATen's fp64 moments are Welford updates: for a
        # count that is no power of two they leave 1e-14 on z, which would make an exact 0 a tiny non-zero 16-bit value
        z = (z * 8).round() / 8
        assert torch.equal(y.cpu(), (z.relu() if relu else z).to(dtype)), (form, slices)
        assert torch.equal(stats.cpu(), rstats.float()), (form, slices)
    for form, slices in _forms(x.shape, groups, True, s2) if backward else []:
        dx, dg, db = GN.gn_backward(dy, x, y, gamma, stats, groups, relu, form=form, slices=slices)
        assert torch.equal(dx.cpu(), grads[0].to(dtype)), (form, slices)
        assert torch.equal(dg.cpu(), grads[1].float()) and torch.equal(db.cpu(), grads[2].float()), (form, slices)


RANDOM = [(3, 5, 7, 24, 8), (2, 8, 8, 128, 1), (4, 16, 64, 264, 33), (1, 40, 40, 64, 64)]


def _ratio(name, got, ref, bound):
    r = ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"err/bound {name}: {r:.3f}")
    return r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("n,h,w,c,groups", RANDOM)
def test_random_against_fp64(n, h, w, c, groups, resident, dtype):
    """Bounds.  half(v) = half an ulp of the one 16-bit rounding of v: u |v| with u = 2^-8 (bf16) / 2^-11 (fp16), and
    the format's fixed spacing below its smallest normal number (2^-25 for fp16).  e = 2^-24 per fp32 rounding on the
    kernel's path (groupnorm.hip's header names them); mean, rstd, c1, c2 are per (sample, group):
    y:      5 roundings (mean, rstd, a = gamma rstd, b = fma(-mean, a, beta), fma(x, a, b)), each relative to a term of
            |x a| + |mean a| + |beta|.
    dx:     10 over mag = rstd (|gamma dz| + |c1| + |xhat c2|): rstd twice (in xhat and as the last factor), x - mean,
            (.) rstd, gamma dz, (.) - c1, fma(-xhat, c2, .), rstd (.), and the roundings of c1 and c2; plus the
            cancellation in x - mean, rstd |c2| |mean| rstd; plus what the fp32 xhat inside S2 does to c2:
            rstd |xhat| dc2, dc2 = group mean of |gamma dz| (3 |xhat| + |mean| rstd) (rstd, x - mean, (.) rstd; mean).
    dgamma: the same four through xhat, and the final fp32 rounding of the double sum: 4 sum |dz xhat| +
            sum |dz| |mean| rstd;  dbeta: 1 (the double sum is exact to 2^-53) over sum |dz|."""
    from can_distributed_pytorch_amd.ops import groupnorm as GN
    torch.manual_seed(c + groups)
    u, e, eps, cg = (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11), 2.0 ** -24, 1e-5, c // groups
    half = lambda v: (u * v.abs()).clamp_min(2.0 ** (-134 if dtype == torch.bfloat16 else -25))
    spread = torch.rand(c, device="cuda") + 0.25
    x = torch.randn(n, h, w, c, device="cuda") * spread + 8 * spread * (2 * torch.rand(c, device="cuda") - 1)
    x[..., cg * (groups // 2):cg * (groups // 2 + 1)] = 1.75      # a constant group: var = 0, rstd = 1 / sqrt(eps)
    x = x.to(dtype)
    gamma, beta = torch.randn(c, device="cuda"), torch.randn(c, device="cuda")
    dy = torch.randn(n, h, w, c, device="cuda").to(dtype)
    fits = lambda backward: resident and GN.plan(x.shape, groups, backward)["bundle"] > 0
    assert not resident or fits(False)                 # every shape here has a resident forward; not all a backward
    ff, fb = (GN.RESIDENT if fits(False) else GN.STREAMED), (GN.RESIDENT if fits(True) else GN.STREAMED)
    y, stats = GN.gn_forward(x, gamma, beta, groups, eps, True, form=ff)
    dx, dg, db = GN.gn_backward(dy, x, y, gamma, stats, groups, True, form=fb)
    y2, stats2 = GN.gn_forward(x, gamma, beta, groups, eps, True, form=ff)
    again = GN.gn_backward(dy, x, y, gamma, stats, groups, True, form=fb)
    assert torch.equal(y, y2) and torch.equal(stats, stats2)
    assert all(torch.equal(p, q) for p, q in zip((dx, dg, db), again))
    z, rstats, grads = _ref(x, gamma, beta, groups, eps, dy, y > 0)
    per_c = lambda t: t.repeat_interleave(cg, 1)[:, None, None, :]             # [N,G] -> [N,1,1,C]
    per_g = lambda t: t.reshape(n, h * w, groups, cg).mean((1, 3))             # [N,H,W,C] -> group means [N,G]
    mean, rstd = per_c(rstats[..., 0]), per_c(rstats[..., 2])
    a, x64 = gamma.double() * rstd, x.double()
    r = [_ratio("y", y, z.relu(), half(z.relu()) + 5 * e * ((x64 * a).abs() + (mean * a).abs() + beta.abs()))]
    dz = dy.double() * (y > 0)
    gdz, xhat = gamma.double() * dz, (x64 - mean) * rstd
    c1, c2 = per_c(per_g(gdz)), per_c(per_g(gdz * xhat))
    dc2 = per_c(per_g(gdz.abs() * (3 * xhat.abs() + mean.abs() * rstd)))
    mag = rstd * (gdz.abs() + c1.abs() + (xhat * c2).abs())
    bound = half(grads[0]) + e * (10 * mag + rstd * c2.abs() * mean.abs() * rstd + rstd * xhat.abs() * dc2)
    r.append(_ratio("dx", dx, grads[0], bound))
    sums = 4 * (dz * xhat).abs().sum((0, 1, 2)) + (dz.abs() * mean.abs() * rstd).sum((0, 1, 2))
    r.append(_ratio("dgamma", dg, grads[1], e * sums))
    r.append(_ratio("dbeta", db, grads[2], e * dz.abs().sum((0, 1, 2))))
    assert max(r) <= 1.0, r


def test_plan():
    from can_distributed_pytorch_amd.ops import groupnorm as GN
    p = GN.plan((1, 40, 40, 64), 64)                   # bundle 32: a 100-KiB tile + 37.25 KiB of reduction scratch
    assert (p["form"], p["bundle"], p["lds"]) == (GN.RESIDENT, 32, 1600 * 64 + 38144)
    p = GN.plan((1, 40, 40, 64), 64, backward=True)    # two tiles do not fit 160 KiB
    assert (p["form"], p["bundle"]) == (GN.STREAMED, 0)
    p = GN.plan((8, 96, 128, 512), 32)
    assert p["form"] == GN.STREAMED and p["spans"] == 2 and p["S"] > 1
    # lcm(cg, 8) rounded up to a 64-byte run: cg = 3 -> 24, cg = 16 -> 32 (48 channels: a ragged last bundle), cg = 128
    assert [GN.plan(s, g)["bundle"] for s, g in (((3, 5, 7, 24), 8), ((2, 8, 16, 48), 3), ((2, 8, 8, 128), 1))] == \
        [24, 32, 128]


def test_refusals():
    from can_distributed_pytorch_amd.ops import _ext, groupnorm as GN
    v = lambda c: torch.ones(c, device="cuda")
    x = lambda *s, d=torch.bfloat16: torch.zeros(*s, device="cuda", dtype=d)
    for args, kw in (((x(1, 2, 2, 12), v(12), v(12), 4, 1e-5, True), {}),                  # C % 8
                     ((x(1, 2, 2, 8), v(8), v(8), 3, 1e-5, True), {}),                     # C % G
                     ((x(1, 1, 1, 8), v(8), v(8), 8, 1e-5, True), {}),                     # one value per group
                     ((x(1, 2, 2, 8), v(8), v(8), 8, -1e-5, True), {}),                    # eps < 0
                     ((x(1, 2, 2, 8), v(8), v(8), 8, float("nan"), True), {}),
                     ((x(1, 2, 2, 8, d=torch.float32), v(8), v(8), 8, 1e-5, True), {}),
                     ((x(1, 2, 2, 8), v(8), v(8), 8, 1e-5, True), {"form": 3}),
                     ((x(1, 2, 2, 8), v(8), v(8), 8, 1e-5, True), {"slices": 65536}),
                     ((x(1, 64, 64, 64), v(64), v(64), 64, 1e-5, True), {"form": GN.RESIDENT})):   # 256 KiB tile
        with pytest.raises(ValueError):
            GN.gn_forward(*args, **kw)
    t, raw = x(1, 2, 2, 16), _ext.require().gn_forward
    p = t.data_ptr()
    ok = dict(x=p, part=p, n=1, h=2, w=2, c=8, g=8, eps=1e-5, dt=0, form=1, slices=1)
    for change, rc in (({"c": 12, "g": 4}, -2), ({"g": 3}, -2), ({"h": 1, "w": 1}, -3), ({"eps": -1.0}, -4),
                       ({"eps": float("nan")}, -4), ({"n": 65536}, -5), ({"form": 3}, -6), ({"slices": 65536}, -6),
                       ({"part": 0}, -6), ({"x": 0}, -7), ({"h": 64, "w": 64, "c": 64, "g": 64, "form": 2}, -8),
                       ({"dt": 2}, -20)):
        a = {**ok, **change}
        with pytest.raises(RuntimeError, match=f"rc={rc}"):
            raw(a["x"], p, p, p, a["part"], p, p, a["n"], a["h"], a["w"], a["c"], a["g"], a["eps"], 1, a["dt"],
                a["form"], a["slices"], 0)
