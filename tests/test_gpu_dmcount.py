"""csrc/otloss.hip against tests/dmcount_reference.py in float64 (README, "DM-Count loss").

The tolerance is not chosen: the same reference run in float32 has an error against float64, and the kernel may be
within 8 times that error, element by element (the 8 covers its other summation order and the MFMA's accumulation),
with a floor of 4 fp32 ulp of the largest magnitude that enters the element:
  L_c    max(N, P)                          L_ot   max |beta| + max |alpha| (two weighted means)
  L_tv   2 N (N (sum a + sum q / N))        g      1 + w_ot 2 max |beta| P / (P^2 + 1e-8) + w_tv 2 N / (P + 1e-8)
  loss   the sum over samples of the terms' magnitudes, weighted.
No element is left out: the inputs are chosen so that no sign argument (P - N, a_m - q_m / N) of the float64 reference
is within 1e-4 / 1e-5 (relative, a hundred times the float32 error and more) of zero, which is asserted on the
reference.  The worst err / bound per case is printed with ``pytest -s`` (profiles/r22/dmcount_errors.txt).
"""
import numpy as np
import pytest
import torch

from dmcount_reference import D8, reference

pytestmark = pytest.mark.gpu

ULP4 = 4 * 2.0 ** -23
W_OT, W_TV = 0.1, 0.01
# (h, w, heads per sample, slots per sample, g pitch, a sample with a map of zeros): the head tile is 16 up to 64 heads,
# 32 up to 256, else 64, so 17 heads are two tiles of 16, 64 / 65 two full tiles of 32 and one head more, 600 nine
# tiles of 64 and a ragged tenth; 17 x 33 is off the MFMA's 16 in both directions
CASES = {"one": (2, 3, [1], [1], None, None), "batch": (5, 7, [3, 0, 17], [3, 2, 17], None, None),
         "tiles": (17, 33, [600], [600], None, None), "edge": (16, 16, [64, 65], [64, 65], None, None),
         "padded": (5, 7, [3, 0, 17], [3, 2, 17], 12, 0)}


def _inputs(name):
    """Per sample: |et| = U[0.5, 1.5] s N / M with s = 0.6 or 1.7 (U[0.5, 1.5] without heads), a quarter of the cells
    negative; the points uniform in the crop, the first two of a sample moved onto cell borders."""
    h, w, heads, _, _, zero = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    et, pts = [], []
    for k, N in enumerate(heads):
        e = rng.uniform(0.5, 1.5, (h, w)) * ((0.6, 1.7)[k % 2] * N / (h * w) if N else 1.0)
        et.append(e * np.where(rng.uniform(size=(h, w)) < 0.25, -1.0, 1.0) * (k != zero))
        p = np.stack([rng.uniform(0, w * D8, N), rng.uniform(0, h * D8, N)], 1)
        p[:2] = np.floor(p[:2] / D8) * D8
        pts.append(p.astype(np.float32))
    return np.stack(et).astype(np.float32), pts


def _target(pts_list, slots, h, w):
    from can_distributed_pytorch_amd.ops.bayes import PointTarget
    begins = np.concatenate([[0], np.cumsum(slots)]).astype(np.int64)
    pts = np.full((begins[-1], 2), np.nan, dtype=np.float32)
    for b, p in zip(begins, pts_list):
        pts[b:b + len(p)] = p
    cnt = torch.tensor([len(p) for p in pts_list], dtype=torch.int32)
    return PointTarget(torch.from_numpy(pts).cuda(), torch.from_numpy(begins).cuda(), cnt.cuda(), len(slots), h, w,
                       h * D8, w * D8)


def _magnitudes(r, N):
    if r["da"] is None:
        return np.array([max(N, float(np.abs(r["dPN"] + N))), 0.0, 0.0]), 1.0
    P, bmax = float(r["P"]), float(np.abs(r["beta"]).max())
    return (np.array([max(N, P), bmax + float(np.abs(r["alpha"]).max()), 2.0 * N]),
            1.0 + W_OT * 2 * bmax * P / (P * P + 1e-8) + W_TV * 2 * N / (P + 1e-8))


@pytest.mark.parametrize("reg,iters", [(10.0, 100), (1.0, 1), (1.0, 100)])
@pytest.mark.parametrize("name", sorted(CASES))
def test_dmcount_loss_against_fp64(name, reg, iters):
    from can_distributed_pytorch_amd.ops.dmcount import dmcount_loss
    h, w, heads, slots, gpitch, _ = CASES[name]
    et, pts = _inputs(name)
    r64 = [reference(e, p, reg, iters, W_OT, W_TV) for e, p in zip(et, pts)]
    r32 = [reference(e, p, reg, iters, W_OT, W_TV, dtype=np.float32) for e, p in zip(et, pts)]
    for r, N in zip(r64, heads):                 # the precondition, on the reference alone: no sign is undefined
        assert abs(r["dPN"]) > 1e-4 * max(N, 1)
        assert r["da"] is None or (np.abs(r["da"]) > 1e-5 * (r["a"] + np.abs(r["a"] - r["da"]))).all()
    target = _target(pts, slots, h, w)
    x = torch.from_numpy(et).cuda()
    loss, g, terms = dmcount_loss(x, target, reg, iters, W_OT, W_TV, gpitch=gpitch)
    again = dmcount_loss(x, target, reg, iters, W_OT, W_TV, gpitch=gpitch)
    assert all(torch.equal(p, q) for p, q in zip((loss, g, terms), again)), "a second call differs"
    g, terms = g.cpu().numpy().astype(np.float64), terms.cpu().numpy().astype(np.float64)
    assert g.shape == (len(heads), h, gpitch or w) and not g[..., w:].any(), "the padding columns are not zero"
    worst, L64, L32, Lmag = {}, 0.0, 0.0, 0.0

    def hold(what, got, want, f32, mag):
        bound = np.maximum(8 * np.abs(np.asarray(f32, dtype=np.float64) - want), ULP4 * mag)
        worst[what] = max(worst.get(what, 0.0), float(np.max(np.abs(got - want) / bound)))

    for i, (a, b, N) in enumerate(zip(r64, r32, heads)):
        tmag, gmag = _magnitudes(a, N)
        hold("terms", terms[i], a["terms"], b["terms"], np.maximum(tmag, 1e-30))
        hold("g", g[i, :, :w], a["g"], b["g"], gmag)
        L64, L32, Lmag = L64 + a["L"], L32 + float(b["L"]), Lmag + tmag @ [1.0, W_OT, W_TV]
    hold("loss", float(loss), L64, L32, Lmag)
    print(f"\nDMCOUNT {name:<6s} reg {reg:g} iters {iters}: worst err / bound " +
          " ".join(f"{k} {v:.3f}" for k, v in worst.items()), end="")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_executor_and_one_step(dtype):
    """head_train_dmcount is head_forward -> dmcount_loss -> head_bwd bit for bit, and one NativeStepper step on a
    64 x 96 crop batch writes the stand-alone loss to flags[1], finite, the same bits in a second run."""
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    from can_distributed_pytorch_amd.ops.dmcount import dmcount_loss
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, preprocess_packed
    with pytest.raises(ValueError):
        NativeStepper("cuda", loss="dmcount", graph=True)
    rng = np.random.default_rng(0)
    items = []
    for flip, n_heads in enumerate((40, 15)):
        img = torch.from_numpy(rng.integers(0, 256, (100, 140, 3), dtype=np.uint8))
        heads = np.stack([rng.integers(0, 140, n_heads), rng.integers(0, 100, n_heads), np.full(n_heads, 2),
                          np.full(n_heads, 8)], 1).astype(np.float32)
        items.append((img, torch.from_numpy(heads), torch.tensor([[int(rng.integers(0, 36)), int(rng.integers(0, 44)),
                                                                   flip]])))
    packed = PackedCollate(crop=(64, 96), gt_from_heads=True)(items)
    x4, target = preprocess_packed(packed, "cuda", dtype=torch.float16 if dtype == "fp16" else torch.bfloat16,
                                   points=True)
    assert target.shape == ("points", 2, 8, 12) and 0 < int(target.cnt.sum()) < 55
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        st = NativeStepper("cuda", dtype=dtype, loss="dmcount", graph=False, lr=1e-5)
        ex = st.ex
        # (random weights this deep underflow fp16 features to 0, and a map of zeros has the count term alone)
        ex.head.bias.data.fill_(0.05)
        b6, _ = ex.forward_features(x4, save=True)              # (the step's own forward)
        want, g, terms = dmcount_loss(ex.head_forward(b6), target)
        assert (terms[:, 1:] != 0).all(), "a sample without its transport and variation terms"
        if not runs:
            ga, gb = ([t.clone() for t in st.grads] for _ in range(2))
            _, _, d1 = ex.head_train_dmcount(b6, target, ga)
            d2 = ex.head_bwd(b6, g, gb)
            assert torch.equal(d1.view(torch.int16), d2.view(torch.int16))
            for i in (ex.head_w_index, ex.head_b_index):
                assert torch.equal(ga[i], gb[i])
        before = st.arena.data.clone()
        loss = st.step(x4, target)
        assert torch.equal(loss.reshape(1), want) and torch.equal(st.flags[1:2], want)
        assert float(st.flags[0]) == 0.0 and np.isfinite(float(want)) and not torch.equal(st.arena.data, before)
        runs.append((loss.clone(), st.arena.data.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
