"""csrc/bayes.hip against the float64 definition of the Bayesian point loss (README, "Bayesian loss"), kept here as one
function, ``reference``, which also returns the error bounds of an fp32 evaluation (u = 2^-24):

  a head logit l = k |x - z|^2 carries 8 roundings (dx; dy, dy^2; the fma; sigma, k, 1 / 2 sigma^2; the product):
  eps = 8 u |l|.  The background's l_0 = k q^2, q = D - dmin, has |dq| <= u (2 D + 3 dmin + |q|) (rho and D rounded,
  dmin^2 4 u, its root 3 u), so eps_0 = u (7 |l_0| + 2 |k| |q| (2 D + 3 dmin)).
  lse_m over C classes: the logits' errors weigh in by their posteriors, the C exponentials (argument rounding and a
  2 u exp: at most u (log C + 2) of the sum), their sequential sum (C - 1) u, the log 2 u log C, the last add u |lse|:
  dlse = sum_n p eps + u (C + 2 + 3 log C) + u |lse|.
  t = l - lse: dt = eps + dlse + u |t|;  p = exp(t) with a 2 u exp: dp = p expm1(dt + 2 u) (+ 2^-126: underflow).
  E_n: dp |et| summed, plus the summation: lanes stride the pixels and a butterfly joins them, depth ceil(M / 64) + 6
  (E_0: 256 threads, butterfly, four waves: ceil(M / 256) + 9).  g_m: |sgn| dp summed, plus a chain of C fmas.
  The loss: the E bounds summed, plus its own sum (depth ceil(N / 256) + 10 + samples).

None of it is fitted to the kernel; the worst err / bound per quantity is printed with ``pytest -s``
(profiles/r21/bayes_errors.txt).  crop_points and head_bwd are held bit for bit.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U, TINY, D8 = 2.0 ** -24, 2.0 ** -126, 8
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for q, r in sorted(_worst.items()):
        print(f"\nBAYES worst err / bound  {q:<5s} {r:.4f}", end="")


def reference(et, pts, ch, cw, sigma, rho):
    """One sample in float64: E [N], E0, g [h, w], L and the bounds bE, bE0, bg of an fp32 evaluation."""
    h, w = et.shape
    M, N = h * w, len(pts)
    et = et.astype(np.float64).ravel()
    if N == 0:
        E0 = et.sum()
        bE0 = (math.ceil(M / 256) + 9) * U * np.abs(et).sum()
        return dict(E=np.zeros(0), E0=E0, g=np.full((h, w), np.sign(E0)), L=abs(E0), bE=np.zeros(0), bE0=bE0,
                    bg=np.zeros((h, w)), margin=abs(E0), signs_safe=bE0 < abs(E0))
    ii, jj = np.divmod(np.arange(M), w)
    z = pts.astype(np.float64)
    d2 = (D8 * jj + D8 / 2 - z[:, :1]) ** 2 + (D8 * ii + D8 / 2 - z[:, 1:]) ** 2          # [N, M]
    k = -1.0 / (2.0 * sigma * sigma)
    l, tgt, depth = k * d2, np.ones(N), np.full(N, math.ceil(M / 64) + 6.0)
    eps = 8 * U * np.abs(l)
    if rho > 0:
        D, dmin = rho * min(ch, cw), np.sqrt(d2.min(0))
        q = D - dmin
        l = np.vstack([l, k * q * q])
        eps = np.vstack([eps, U * (7 * np.abs(l[-1]) + 2 * abs(k) * np.abs(q) * (2 * D + 3 * dmin))])
        tgt, depth = np.append(tgt, 0.0), np.append(depth, math.ceil(M / 256) + 9.0)
    C = l.shape[0]
    mx = l.max(0)
    lse = mx + np.log(np.exp(l - mx).sum(0))
    p = np.exp(l - lse)
    dlse = (p * eps).sum(0) + U * (C + 2 + 3 * math.log(C)) + U * np.abs(lse)
    dp = p * np.expm1(eps + dlse + U * np.abs(l - lse) + 2 * U) + TINY
    E = p @ et
    bE = dp @ np.abs(et) + depth * U / (1 - depth * U) * ((p + dp) @ np.abs(et))
    sg = np.sign(E - tgt)
    out = dict(E=E[:N], bE=bE[:N], E0=E[N] if rho > 0 else 0.0, bE0=bE[N] if rho > 0 else 0.0, L=np.abs(E - tgt).sum(),
               g=(sg @ p).reshape(h, w), bg=(np.abs(sg) @ dp + C * U / (1 - C * U) * (np.abs(sg) @ (p + dp))).reshape(h, w))
    out.update(margin=np.abs(E - tgt).min(), signs_safe=bool((bE < np.abs(E - tgt)).all()))
    return out


def _ratio(q, err, bound):
    r = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)))) if np.size(err) else 0.0
    _worst[q] = max(_worst.get(q, 0.0), r)
    return r


def _target(pts_list, slots, h, w):
    """PointTarget of samples with the given points; slots[s] >= len(pts_list[s]) (the rest of a sample's slots unused)."""
    from can_distributed_pytorch_amd.ops.bayes import PointTarget
    begins = np.concatenate([[0], np.cumsum(slots)]).astype(np.int64)
    pts = np.full((begins[-1], 2), np.nan, dtype=np.float32)
    for b, p in zip(begins, pts_list):
        pts[b:b + len(p)] = p
    cnt = torch.tensor([len(p) for p in pts_list], dtype=torch.int32)
    return PointTarget(torch.from_numpy(pts).cuda(), torch.from_numpy(begins).cuda(), cnt.cuda(), len(slots), h, w,
                       h * D8, w * D8), begins


# (h, w, heads per sample, slots per sample): 17 x 33 crosses a 16 x 16 tile edge, 257 / 600 the 256-point LDS chunk;
# the batch has its zero-head sample in the middle, with unused slots
CASES = [(2, 3, [1], [1]), (2, 3, [5], [5]), (17, 33, [257], [257]), (17, 33, [600], [600]), (16, 16, [0], [0]),
         (17, 33, [257, 0, 5], [257, 3, 5])]


def _inputs(rng, heads, h, w, s):
    """Per sample, in order: et = U[0.5, 1.5] s N / (h w) (U[-1, 1] without heads), then the points' x, then their y."""
    et, pts = [], []
    for N in heads:
        et.append(rng.uniform(0.5, 1.5, (h, w)) * s * N / (h * w) if N else rng.uniform(-1, 1, (h, w)))
        pts.append(np.stack([rng.uniform(0, w * D8, N), rng.uniform(0, h * D8, N)], 1).astype(np.float32))
    return np.stack(et).astype(np.float32), pts


@pytest.mark.parametrize("rho", [0.15, 0.0])
@pytest.mark.parametrize("h,w,heads,slots", CASES)
def test_bayes_loss_against_fp64(h, w, heads, slots, rho):
    from can_distributed_pytorch_amd.ops.bayes import bayes_loss
    ch, cw, failed = h * D8, w * D8, []
    for seed in range(3):
        for s in (0.5, 2.0):
            et, pts = _inputs(np.random.default_rng(seed), heads, h, w, s)
            refs = [reference(e, p, ch, cw, 8.0, rho) for e, p in zip(et, pts)]
            # the precondition, on the reference alone: no sign can flip within the fp32 error (every |E - target| is
            # at least 1e-3 and above its own bound)
            assert min(r["margin"] for r in refs) >= 1e-3 and all(r["signs_safe"] for r in refs)
            target, begins = _target(pts, slots, h, w)
            loss, g, E = bayes_loss(torch.from_numpy(et).cuda(), target, sigma=8.0, bg_ratio=rho)
            again = bayes_loss(torch.from_numpy(et).cuda(), target, sigma=8.0, bg_ratio=rho)
            assert all(torch.equal(a, b) for a, b in zip((loss, g, E), again)), "a second call differs"
            E, g = E.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
            rs = []
            for i, r in enumerate(refs):
                N, b = heads[i], begins[i]
                assert not E[b + N:begins[i + 1]].any(), "a slot without a head is not 0"
                rs += [_ratio("E", np.abs(E[b:b + N] - r["E"]), r["bE"]),
                       _ratio("E0", np.abs(E[begins[-1] + i] - r["E0"]), r["bE0"]),
                       _ratio("g", np.abs(g[i] - r["g"]), r["bg"])]
            L = sum(r["L"] for r in refs)
            bL = sum(r["bE"].sum() + r["bE0"] for r in refs) + (math.ceil(max(heads) / 256) + 10 + len(heads)) * U * L
            rs.append(_ratio("loss", abs(float(loss) - L), bL))
            if not max(rs) <= 1.0:
                failed.append(f"seed {seed} s {s}: err / bound (E, E0, g per sample, loss) = {rs}")
    assert not failed, "\n".join(failed)


def _ref_points(heads, row, ch, cw):
    """The README's definition in numpy: the window's records, in table order, as fp32 crop pixels."""
    _, H0, W0, _, flip, y0, x0, s7 = row
    if s7 == 1:
        sh, sw = min(ch, H0 // D8 * D8), min(cw, W0 // D8 * D8)
        th, tw = sh, sw
    else:
        sh, sw, th, tw = s7 >> 32, s7 & 0xffffffff, ch, cw
    c, r = heads[:, 0].astype(np.int64) - x0, heads[:, 1].astype(np.int64) - y0
    keep = (c >= 0) & (c < sw) & (r >= 0) & (r < sh)
    zx = (((2 * c + 1) * tw).astype(np.float64) / np.float64(2 * sw)).astype(np.float32)
    zy = (((2 * r + 1) * th).astype(np.float64) / np.float64(2 * sh)).astype(np.float32)
    if flip:
        zx = (np.float64(tw) - zx.astype(np.float64)).astype(np.float32)
    return np.stack([zx, zy], 1)[keep]


def test_crop_points_bit_for_bit():
    from can_distributed_pytorch_amd.ops.bayes import crop_points
    rng = np.random.default_rng(0)
    ch, cw = 32, 40

    def table(n, H0, W0):
        return np.stack([rng.integers(0, W0, n), rng.integers(0, H0, n), np.full(n, 2), np.full(n, 8)], 1)
    # image A 140 x 170 with 300 heads (two chunks), B 20 x 150 (smaller than the crop: 16 valid rows), C with its five
    # heads in a corner the window misses; A's samples: both flips unscaled, sh / ch = 4 and 0.25, two crops of one range
    heads = np.concatenate([table(300, 140, 170), table(40, 20, 150), table(5, 20, 20)]).astype(np.float32)
    A, B, Cc = (0, 300, 140, 170), (300, 40, 20, 150), (340, 5, 140, 170)
    samples = [(A, 3, 2, 0, 1), (A, 50, 100, 1, 1), (A, 5, 7, 1, (128 << 32) | 160), (A, 60, 80, 0, (8 << 32) | 10),
               (A, 60, 80, 1, (8 << 32) | 10), (B, 0, 45, 0, 1), (B, 0, 90, 1, 1), (Cc, 100, 100, 0, 1)]
    desc = np.array([[0, im[2], im[3], 3, fl, y0, x0, s7] for im, y0, x0, fl, s7 in samples], dtype=np.int64)
    ranges = np.array([[im[0], im[1]] for im, *_ in samples], dtype=np.int64)
    t = crop_points(torch.from_numpy(heads).cuda(), torch.from_numpy(ranges).cuda(), torch.from_numpy(desc).cuda(),
                    len(samples), ch, cw)
    pts, begins, cnt = (x.cpu().numpy() for x in t.tensors())
    assert begins.tolist() == np.concatenate([[0], np.cumsum(ranges[:, 1])]).tolist() and t.shape == ("points", 8, 4, 5)
    for i, row in enumerate(desc):
        want = _ref_points(heads[ranges[i, 0]:ranges[i, 0] + ranges[i, 1]], row.tolist(), ch, cw)
        assert cnt[i] == len(want) and (i != 7 or cnt[i] == 0)
        assert pts[begins[i]:begins[i] + cnt[i]].tobytes() == want.tobytes(), f"sample {i}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,pitch,wv", [(1, 2, 3, 0), (1, 17, 64, 33), (1, 260, 128, 0)])   # the last: P > 1024 * 32,
# the grid's cap, so lanes sum two pixels and a product fused into a sum would show
def test_head_bwd_equals_head_train(dtype, n, h, pitch, wv):
    from can_distributed_pytorch_amd.ops import _ext
    C, st = _ext.require(), _ext.stream_ptr()
    gen = torch.Generator().manual_seed(1)
    P, dt, gscale = n * h * pitch, int(dtype == torch.float16), 0.37
    b6 = torch.randn(P, 64, generator=gen).to(dtype).cuda()
    w, b = torch.randn(64, generator=gen).cuda(), torch.randn(1, generator=gen).cuda()
    gt = torch.rand(n, h, pitch, generator=gen).cuda()
    if wv:
        gt[..., wv:] = 0
    nblk = max(1, min(1024, (P * 8 + 255) // 256))
    et, part, loss = torch.empty(P, device="cuda"), torch.empty(nblk * 66, device="cuda"), torch.empty(1, device="cuda")
    dy, dw, db = (torch.empty(s, device="cuda", dtype=t) for s, t in (((P, 64), dtype), (64, torch.float32), (1, torch.float32)))
    C.head_train(b6.data_ptr(), w.data_ptr(), b.data_ptr(), gt.data_ptr(), et.data_ptr(), dy.data_ptr(), part.data_ptr(),
                 nblk, dw.data_ptr(), db.data_ptr(), loss.data_ptr(), P, gscale, 0.0, 0, 0, dt, st, pitch if wv else 0, wv)
    g = 2 * (et - gt.reshape(-1))                                # fp32, the doubling exact
    dw1, db1, dy2 = dw.clone(), db.clone(), torch.empty_like(dy)
    for beta, k in ((0.0, 1), (1.0, 2)):                         # beta = 1 adds to the slots: exactly twice
        C.head_bwd(b6.data_ptr(), w.data_ptr(), g.data_ptr(), dy2.data_ptr(), part.data_ptr(), nblk, dw.data_ptr(),
                   db.data_ptr(), loss.data_ptr(), P, gscale, beta, 0, dt, st)
        assert torch.equal(dy2.view(torch.int16), dy.view(torch.int16))
        assert torch.equal(dw, k * dw1) and torch.equal(db, k * db1)


def test_one_bayes_step():
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    from can_distributed_pytorch_amd.ops.bayes import bayes_loss
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, preprocess_packed
    with pytest.raises(ValueError):
        NativeStepper("cuda", loss="bayes", graph=True)
    rng = np.random.default_rng(0)
    items = []
    for flip, n_heads in enumerate((30, 12)):
        img = torch.from_numpy(rng.integers(0, 256, (60, 80, 3), dtype=np.uint8))
        heads = np.stack([rng.integers(0, 80, n_heads), rng.integers(0, 60, n_heads), np.full(n_heads, 2),
                          np.full(n_heads, 8)], 1).astype(np.float32)
        items.append((img, torch.from_numpy(heads), torch.tensor([[int(rng.integers(0, 28)), int(rng.integers(0, 32)),
                                                                   flip]])))
    packed = PackedCollate(crop=(32, 48), gt_from_heads=True)(items)
    x4, target = preprocess_packed(packed, "cuda", points=True)
    assert target.shape == ("points", 2, 4, 6) and 0 < int(target.cnt.sum()) < 42
    torch.manual_seed(0)
    st = NativeStepper("cuda", loss="bayes", graph=False, lr=1e-5)
    b6, _ = st.ex.forward_features(x4, save=True)               # (the step's own forward)
    want = bayes_loss(st.ex.head_forward(b6), target)[0]
    before = st.arena.data.clone()
    loss = st.step(x4, target)
    assert torch.equal(loss.reshape(1), want) and float(st.flags[0]) == 0.0
    assert not torch.equal(st.arena.data, before)
