"""tests/density_reference.py against independent code, on the CPU: sigmas_ref against scipy's KD-tree, splat_ref
against scipy.ndimage.gaussian_filter on a delta, the upsample against torch's bilinear interpolate in fp64, render_ref
against the CPU recipe make_synthetic_batch(1, ...); that the shared inputs meet their conditions (no radius-ambiguous
head, the splat bound at or below 1e-4 of the value); and that the bounds have teeth: seven wrong variants of the
references each leave an element outside its bound by the factor asserted here (printed with ``pytest -s``, recorded in
profiles/r15/README.md).
"""
import numpy as np
import pytest
import torch

import density_reference as R

EPS64 = 2.0 ** -53


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------- against independent code
@pytest.mark.parametrize("name", list(R.knn_cases()))
def test_sigmas_ref_matches_kdtree(name):
    from can_distributed_pytorch_amd.data.density import knn_sigmas
    pts = R.knn_cases()[name]
    want = knn_sigmas(pts.astype(np.float64), (R.KNN_H, R.KNN_W))
    got = R.sigmas_ref(pts, R.KNN_H, R.KNN_W)
    err = np.abs(got - want).max()
    print(f"\nsigmas_ref vs KDTree {name}: max abs diff {err:.3g}")
    assert err <= 8 * EPS64 * np.abs(want).max()


def test_sigmas_ref_single_head():
    assert R.sigmas_ref(np.array([[3.0, 4.0]], dtype=np.float32), 48, 80).tolist() == [16.0]


def _scipy_splat(pts, sig, H, W):
    from scipy.ndimage import gaussian_filter
    out = np.zeros((H, W))
    for (x, y), s in zip(pts, sig):
        if x < 0 or y < 0 or int(x) >= W or int(y) >= H:
            continue
        delta = np.zeros((H, W))
        delta[int(y), int(x)] = 1.0
        out += gaussian_filter(delta, s, mode="constant") if s > 0 else delta
    return out


@pytest.mark.parametrize("name", ["n=2", "n=5", "n=257", "duplicate", "coincident", "fixed4_edges", "fixed4_overlap",
                                  "fixed0.3_edges"])
def test_splat_ref_matches_gaussian_filter(name):
    """fp64 sigmas, one head at a time through gaussian_filter(delta, sigma, mode="constant") and summed."""
    H, W = R.KNN_H, R.KNN_W
    if name.startswith("fixed"):
        pts = R.overlap_heads() if name.endswith("overlap") else np.concatenate([R.edge_heads(H, W), R.INTERIOR])
        sig = np.full(len(pts), float(name[5:].split("_")[0]))
    else:
        pts = R.knn_cases()[name]
        sig = R.sigmas_ref(pts, H, W)
    got = R.splat_ref(pts, sig, H, W)
    want = _scipy_splat(pts, sig, H, W)
    err = np.abs(got.value - want).max()
    print(f"\nsplat_ref vs gaussian_filter {name}: max abs diff {err:.3g} (peak {want.max():.3g})")
    assert err <= 64 * EPS64 * want.max()


@pytest.mark.parametrize("hn,wn", [(1, 1), (2, 3), (3, 5), (8, 12)])
def test_upsample_matches_torch_bilinear(hn, wn):
    g = torch.Generator().manual_seed(hn * 10 + wn)
    nz = torch.rand(2, 3, hn, wn, generator=g, dtype=torch.float64)
    want = torch.nn.functional.interpolate(nz, size=(16 * hn, 16 * wn), mode="bilinear", align_corners=False).numpy()
    got = R.upsample16(nz.numpy())
    assert np.abs(got - want).max() <= 4 * EPS64


@pytest.mark.parametrize("h,w,seed,heads", R.SYNTH_CASES)
def test_render_ref_matches_cpu_recipe(h, w, seed, heads):
    """The fp32 CPU recipe for batch = 1 against render_ref(splat_ref(points, 4.0), noise) with the points and the
    noise redrawn from the seed: image within 2e-6, every ground-truth cell within 2e-6 relative (a cell the reference
    has at 0, which no footprint reaches, is exactly 0 in the recipe)."""
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch
    img, gt = make_synthetic_batch(1, h, w, seed=seed, heads=heads)
    ref, sp = R.synthetic_ref(seed, h, w, heads)
    assert heads[0] <= len(R.draw_synthetic(seed, h, w, heads)[0]) <= heads[1]
    e_img = np.abs(img.numpy().astype(np.float64) - ref.img).max()
    got_gt, pos = gt.numpy().astype(np.float64)[:, 0], ref.gt > 0
    assert pos.any() and not got_gt[~pos].any()
    e_gt = (np.abs(got_gt - ref.gt)[pos] / ref.gt[pos]).max()
    print(f"\nCPU recipe vs render_ref {h}x{w} seed {seed}: image {e_img:.3g}, gt {e_gt:.3g} relative")
    assert e_img <= 2e-6
    assert e_gt <= 2e-6


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("name", list(R.knn_cases()))
def test_knn_inputs_have_no_ambiguous_radius(name):
    """No in-image head has 4 sigma + 0.5 within 1e-4 relative of an integer: the kernel's fp32 sigma (8 u relative,
    about 5e-7) cannot pick another radius than the fp64 one.  The allowed share of such heads is zero."""
    pts = R.knn_cases()[name]
    inside = R.in_image(pts, R.KNN_H, R.KNN_W)
    margin = R.radius_margin(R.sigmas_ref(pts, R.KNN_H, R.KNN_W))[inside]
    print(f"\nradius margin {name}: least {margin.min():.3g} over {inside.sum()} in-image heads of {len(pts)}")
    assert int((margin < 1e-4).sum()) == 0
    if len(pts) >= 255:
        assert 0.1 < 1.0 - inside.mean() < 0.3            # about a fifth of the heads lie outside


def _all_splat_refs():
    for name, (H, W, s, max_r, pts, _) in {**R.SPLAT_CASES, **R.LDS_CASES}.items():
        yield name, R.splat_ref(pts, np.float32(s), H, W, max_r)
    for name, pts in R.knn_cases().items():
        yield name, R.splat_ref(pts, _f32(R.sigmas_ref(pts, R.KNN_H, R.KNN_W)), R.KNN_H, R.KNN_W)
    yield "n=1", R.splat_ref(R.INTERIOR, _f32(R.sigmas_ref(R.INTERIOR, R.KNN_H, R.KNN_W)), R.KNN_H, R.KNN_W)
    h, w, _, heads = R.SYNTH_CASES[2]                       # the sigma-4 splats of the generator cases
    for hh, ww, seed, hd in R.SYNTH_CASES + [(h, w, 11, heads), (h, w, 12, heads)]:
        yield f"generator {hh}x{ww} seed {seed}", R.synthetic_ref(seed, hh, ww, hd)[1]


def test_splat_bound_stays_under_the_ceiling():
    """With C_SPLAT the bound is at most 1e-4 of the value (the relative tolerance of
    test_density_gpu_large_radius_matches_cpu) at every in-footprint element of every case of the GPU file: fixed sigma,
    LDS sizes, kNN, the single head that set C_SPLAT and the generator's splats.  Every in-footprint value is a normal
    fp32 number."""
    worst = 0.0
    for name, sp in _all_splat_refs():
        m = sp.support > 0
        assert m.any(), name
        r = (sp.bound()[m] / sp.value[m]).max()
        worst = max(worst, r)
        assert r <= 1e-4, (name, r)
        assert sp.value[m].min() > 2.0 ** -126, name
    print(f"\nsplat bound / value, worst over the cases: {worst:.3g} (ceiling 1e-4)")


def test_sigma_bound_holds_for_an_fp32_emulation():
    """The kernel's arithmetic in numpy fp32 (products and sums rounded separately) stays inside 8 u sigma."""
    worst = 0.0
    for name, pts in R.knn_cases().items():
        p = pts.astype(np.float32)
        dx, dy = p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]
        v = np.sort(dx * dx + dy * dy, axis=1)
        d = np.sqrt(v[:, 1:min(4, len(p))])
        s = np.zeros(len(p), dtype=np.float32)
        for k in range(d.shape[1]):
            s = s + d[:, k]
        got = np.float32(0.1) * s
        ref = R.sigmas_ref(pts, R.KNN_H, R.KNN_W)
        worst = max(worst, R.worst_ratio(np.abs(got - ref), R.SIGMA_ULPS * R.U * ref))
    print(f"\nfp32 emulation of the sigma chain: worst err / (8 u sigma) {worst:.3g}")
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------- teeth
def _splat_factor(ref, bad_value):
    m = ref.support > 0                    # inside the true footprints; outside them any write at all fails (+0 bits)
    return R.worst_ratio(np.abs(bad_value - ref.value)[m], ref.bound()[m])


def test_bounds_have_teeth():
    """Each wrong variant, built here from the pieces of the reference, leaves at least one element outside its bound
    by the factor asserted below (the measured factors are printed).  The splat factors count only elements inside the
    true footprints: a larger radius or a clamped head also writes outside them, where the GPU test demands +0 bits."""
    f = {}
    s4 = np.float32(4.0)
    H, W, _, _, interior, _ = R.SPLAT_CASES["s4_interior"]
    f["R off by one"] = _splat_factor(R.splat_ref(interior, s4, H, W),
                                      R.splat_ref(interior, s4, H, W, radii=np.array([17])).value)
    edges = R.SPLAT_CASES["s4_edges"][4]
    ref = R.splat_ref(edges, s4, H, W)
    # both 1-D factors normalised over the clipped window: the head's clipped contribution sums to 1
    singles = [R.splat_ref(edges[i:i + 1], s4, H, W).value for i in np.flatnonzero(R.in_image(edges, H, W))]
    f["normaliser over the clipped window (corner heads)"] = _splat_factor(ref, sum(v / v.sum() for v in singles))
    clamped = np.stack([np.clip(edges[:, 0], 0, W - 1), np.clip(edges[:, 1], 0, H - 1)], 1)
    f["out-of-image head clamped, not skipped"] = _splat_factor(ref, R.splat_ref(clamped, s4, H, W).value)

    pts = R.knn_points(257)
    ref = R.sigmas_ref(pts, R.KNN_H, R.KNN_W)
    bad = 0.1 * R.sorted_distances(pts)[:, [1, 2, 4]].sum(axis=1)
    f["one neighbour missed (d1 + d2 + d4)"] = R.worst_ratio(np.abs(bad - ref), R.SIGMA_ULPS * R.U * ref)
    least = min(R.worst_ratio(np.abs(bad[i] - ref[i]), R.SIGMA_ULPS * R.U * ref[i]) for i in (255, 256))
    f["  the same, the least of heads 255 and 256 alone"] = least

    dens, noise = R.render_inputs(2, 32, 48, seed=2, variant="scaled")
    ref = R.render_ref(dens, noise)
    bad = R.normalise(R.blend(R.upsample16(noise), dens, np.full(2, ref.dmax[0])))
    f["dmax of image 0 used for image 1 (bf16 bound)"] = R.worst_ratio(np.abs(bad - ref.img), ref.img_bound("bf16"))

    # lin_tap without min(x0 + 1, in - 1): the weight of the second tap is 0 wherever the clamp acts, so a value changes
    # only through what the tap reads.  After the last noise row of the last channel of the last image that is the
    # NaN the GPU test puts behind the grid: top + (NaN - top) * 0 = NaN, and fmaxf(NaN, 0) = 0 before the normalise.
    dens, noise = R.render_inputs(1, 16, 16, seed=1)
    ref = R.render_ref(dens, noise)
    v = R.blend(R.upsample16(noise), dens, ref.dmax)
    v[-1, 2, -8:, :] = 0.0
    f["second tap read from the NaN guard (bf16 bound)"] = R.worst_ratio(np.abs(R.normalise(v) - ref.img),
                                                                         ref.img_bound("bf16"))

    dens, noise = R.render_inputs(3, 48, 80, seed=3)
    ref = R.render_ref(dens, noise)
    bad = ref.gt - dens.astype(np.float64)[:, 7::8, 7::8]
    f["one of the 64 pool terms dropped"] = R.worst_ratio(np.abs(bad - ref.gt), ref.gt_bound)
    for k, v in f.items():
        print(f"\nTEETH {k}: err / bound = {v:.4g}", end="")
    print()
    assert f["R off by one"] >= 20
    assert f["normaliser over the clipped window (corner heads)"] >= 1e5
    assert f["out-of-image head clamped, not skipped"] >= 1e5
    assert f["one neighbour missed (d1 + d2 + d4)"] >= 1e5 and least >= 1000
    assert f["dmax of image 0 used for image 1 (bf16 bound)"] >= 10
    assert f["second tap read from the NaN guard (bf16 bound)"] >= 10
    assert f["one of the 64 pool terms dropped"] >= 100


def test_half_ulp16_is_the_format_spacing():
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        x = torch.tensor([0.3, 1.0, 1.99, 2.5, 1e-3], dtype=torch.float64)
        lo = x.to(dt).double()
        nxt = torch.nextafter(lo.to(dt), torch.tensor(float("inf"), dtype=dt)).double()
        assert np.allclose(R.half_ulp16(lo.numpy(), name), ((nxt - lo) / 2).numpy(), rtol=0, atol=0)
