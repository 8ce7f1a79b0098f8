"""The kernels that make the ground truth, through their raw entry points C.density_map and C.synth_render, against
the plain fp64 references of tests/density_reference.py: the sigma the kNN kernel writes (elementwise, 8 u), the
radius it implies, the splat within its bound map and +0 bits outside every footprint, the three dynamic-LDS sizes,
the synthetic renderer's gt, per-image dmax and 16-bit image, and make_synthetic_batch_gpu end to end against the
recipe redrawn from the seed.

Every output a kernel writes is pre-filled (NaN, NaN bits, 0xFFFF words), the splat's accumulator apart, which must
start at zero.  The noise grid is followed by NaN in the same allocation: a row or column tap that is not clamped
reads it for the last channel of the last image and turns those pixels into clip(NaN) = 0.  The bounds are derived in
density_reference.py and shown on the CPU to notice seven wrong variants (tests/test_density_reference_cpu.py).
Measured err / bound: profiles/r15/density_errors.txt.
"""
import functools

import numpy as np
import pytest
import torch

import density_reference as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
NAN = float("nan")
_worst = {}          # (quantity, case) -> worst err / bound seen in this session
_rel = {}            # splat case -> worst err / value inside the footprints


def _name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp16"


def _note(failed, q, case, ratio):
    _worst[(q, case)] = max(_worst.get((q, case), 0.0), ratio)
    if not ratio <= 1.0:
        failed.append(f"{case} {q}: err / bound = {ratio:.4g}")


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module: the worst err / bound per quantity and case (shown with ``pytest -s``).  splat_c1 is the
    splat's error over its bound map at C_SPLAT = 1, the figure C_SPLAT was set from."""
    yield
    for (q, case), r in _worst.items():
        print(f"\nDENSITY {case:<28s} {q:<9s} worst err/bound {r:.4f}", end="")
    for case, r in _rel.items():
        print(f"\nDENSITY {case:<28s} splat     worst err/value {r:.3g}", end="")
    c1 = [r for (q, _), r in _worst.items() if q == "splat_c1"]
    if c1:
        print(f"\nDENSITY worst splat err / (bound map at C_SPLAT = 1) over all cases: {max(c1):.4f}", end="")
    print()


@pytest.fixture(scope="module")
def ext():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require(), _ext


def _dt(dtype):
    from can_distributed_pytorch_amd.ops.conv import dt_code
    return dt_code(dtype)


def _full(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------------ density_map
def _density(ext, pts, H, W, fixed=0.0, max_r=0):
    """(sigma_ws, out) of one density_map call: sigma_ws pre-filled with NaN, out zero."""
    C, X = ext
    p = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).cuda()
    sig = _full((len(pts),), NAN)
    out = torch.zeros(H, W, dtype=torch.float32, device="cuda")
    C.density_map(p.data_ptr(), len(pts), H, W, sig.data_ptr(), out.data_ptr(), max_r, X.stream_ptr(), fixed)
    torch.cuda.synchronize()
    return sig.cpu().numpy(), out.cpu().numpy()


def _check_splat(failed, case, out, sp, heads_sum=None):
    """out against splat_ref's value within its bound map; +0 bits outside the support map, nonzero inside."""
    bits = out.view(np.int32)
    if bits[sp.support == 0].any():
        failed.append(f"{case}: {int((bits[sp.support == 0] != 0).sum())} elements outside every footprint are not +0")
    if not (out[sp.support > 0] != 0).all():
        failed.append(f"{case}: a zero inside a footprint")
    err = np.abs(out.astype(np.float64) - sp.value)
    _note(failed, "splat", case, R.worst_ratio(err, sp.bound()))
    _note([], "splat_c1", case, R.worst_ratio(err, sp.bound(1.0)))
    _rel[case] = max(_rel.get(case, 0.0), float((err[sp.support > 0] / sp.value[sp.support > 0]).max()))
    if heads_sum is not None:
        assert abs(sp.value.sum() - heads_sum) <= 1e-12 * heads_sum, case          # the case is what it claims to be
        _note(failed, "sum", case, abs(out.astype(np.float64).sum() - heads_sum) / sp.bound().sum())


@pytest.mark.parametrize("name", list(R.knn_cases()))
def test_knn_sigma_radius_and_map(ext, name):
    """sigma_ws elementwise within 8 u of sigmas_ref (out-of-image heads included: they are written, and they count as
    neighbours); the radius of the kernel's sigma is the fp64 one for every in-image head; the map within the bound
    of splat_ref fed the kernel's own sigmas."""
    pts = R.knn_cases()[name]
    H, W = R.KNN_H, R.KNN_W
    sig, out = _density(ext, pts, H, W)
    ref = R.sigmas_ref(pts, H, W)
    failed = []
    assert not np.isnan(sig).any(), "a sigma was not written"
    _note(failed, "sigma", name, R.worst_ratio(np.abs(sig.astype(np.float64) - ref), R.SIGMA_ULPS * R.U * ref))
    inside = R.in_image(pts, H, W)
    if not np.array_equal(R.radius_f32(sig)[inside], R.radius_f64(ref)[inside]):
        failed.append(f"{name}: a radius differs from the fp64 one")
    _check_splat(failed, name, out, R.splat_ref(pts, sig, H, W))
    if name == "coincident":
        want = np.zeros((H, W), dtype=np.float32)
        want[7, 10] = 4.0
        assert (sig == 0).all() and np.array_equal(out.view(np.int32), want.view(np.int32))
    if name == "duplicate":
        assert sig[0] == sig[5] and ref[0] == ref[5]
    assert not failed, "\n".join(failed)


def test_knn_single_head(ext):
    """n = 1: sigma = (H + W) / 8 = 16, R = 64, the footprint is the whole 48 x 80 image."""
    sig, out = _density(ext, R.INTERIOR, R.KNN_H, R.KNN_W)
    assert sig.tolist() == [16.0]
    failed = []
    _check_splat(failed, "n=1", out, R.splat_ref(R.INTERIOR, sig, R.KNN_H, R.KNN_W))
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("name", list(R.SPLAT_CASES))
def test_splat_fixed_sigma(ext, name):
    """The fixed-sigma path (every synthetic batch takes it): the fill kernel writes the sigma to every head, the map is
    within the bound of splat_ref; max_r caps the radius and the normaliser with it; the sum of a map whose footprints
    lie inside the image is the number of heads within the summed bound; R = 0 gives exactly 1.0."""
    H, W, s, max_r, pts, whole = R.SPLAT_CASES[name]
    sig, out = _density(ext, pts, H, W, fixed=s, max_r=max_r)
    assert (sig == np.float32(s)).all()
    failed = []
    sp = R.splat_ref(pts, sig, H, W, max_r)
    _check_splat(failed, name, out, sp, heads_sum=float(len(pts)) if whole else None)
    if s == 0.124:
        assert set(np.unique(out).tolist()) == {0.0, 1.0} and out.sum() == R.in_image(pts, H, W).sum()
    assert not failed, "\n".join(failed)


def test_density_map_gpu_without_points(ext):
    from can_distributed_pytorch_amd.data.density import density_map_gpu
    out = density_map_gpu(np.zeros((0, 2)), 48, 80)
    assert out.shape == (48, 80) and not out.view(torch.int32).any()
    C, X = ext                                                  # the raw entry point: n = 0 launches nothing
    canary = _full((48, 80), 7.0)
    C.density_map(0, 0, 48, 80, 0, canary.data_ptr(), 0, X.stream_ptr(), 0.0)
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all())


@pytest.mark.parametrize("name", list(R.LDS_CASES))
def test_splat_dynamic_lds_above_64k(ext, name):
    """(H + W) * 4 bytes of weight tables: 65664 (the first size that needs hipFuncSetAttribute) and 153600 (the largest
    accepted), sigma-4 heads, one in the last column."""
    H, W, s, max_r, pts, _ = R.LDS_CASES[name]
    assert (H + W) * 4 == int(name.split("_")[1])
    sig, out = _density(ext, pts, H, W, fixed=s, max_r=max_r)
    failed = []
    _check_splat(failed, name, out, R.splat_ref(pts, sig, H, W, max_r))
    assert not failed, "\n".join(failed)


def test_splat_refuses_more_than_150k_of_lds(ext):
    C, X = ext
    H, W = R.LDS_REFUSED
    assert (H + W) * 4 > 150 * 1024 >= (H + W - 16) * 4
    p = torch.tensor([[5.0, 5.0], [100.0, 3.0]], device="cuda")
    sig, out = _full((2,), NAN), _full((H, W), 7.0)
    for fixed in (0.0, 4.0):
        with pytest.raises(RuntimeError, match="density_map"):
            C.density_map(p.data_ptr(), 2, H, W, sig.data_ptr(), out.data_ptr(), 0, X.stream_ptr(), fixed)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool(torch.isnan(sig).all())


# ----------------------------------------------------------------------------------------------------- synth_render
def _render(ext, dens, noise, dtype):
    """(x4 words [n, H, W, 4] int16, gt, dmax) of one synth_render call on pre-filled outputs; the noise grid is
    followed by a guard of NaN in its allocation."""
    C, X = ext
    n, H, W = dens.shape
    d = torch.from_numpy(dens).cuda()
    nz = _full((noise.size + W // 16 + 2,), NAN)
    nz[:noise.size] = torch.from_numpy(noise).reshape(-1).cuda()
    x4 = _full((n, H, W, 4), -1, torch.int16)
    gt = _full((n, H // 8, W // 8), NAN)
    dmax = _full((n,), NAN)
    C.synth_render(d.data_ptr(), nz.data_ptr(), dmax.data_ptr(), x4.data_ptr(), gt.data_ptr(), n, H, W, _dt(dtype),
                   X.stream_ptr())
    torch.cuda.synchronize()
    return x4.cpu().numpy(), gt.cpu().numpy(), dmax.cpu().numpy()


def _check_render(failed, case, dtype, x4, gt, ref, extra_img=0.0, extra_gt=0.0):
    dt = _name(dtype)
    img, ch3 = R.words_to_f64(x4, dt)
    if ch3.any():
        failed.append(f"{case} {dt}: channel 3 is not the word 0 everywhere")
    if np.isnan(gt).any() or np.isnan(img).any():
        failed.append(f"{case} {dt}: an element was not written")
    _note(failed, "gt", f"{case} {dt}", R.worst_ratio(np.abs(gt.astype(np.float64) - ref.gt), ref.gt_bound + extra_gt))
    _note(failed, "image", f"{case} {dt}", R.worst_ratio(np.abs(img - ref.img), ref.img_bound(dt, extra_img)))


def _render_case(ext, shape, dtype, variant=None):
    n, H, W = shape
    dens, noise = R.render_inputs(n, H, W, seed=n * H + W, variant=variant)
    x4, gt, dmax = _render(ext, dens, noise, dtype)
    ref = R.render_ref(dens, noise)
    failed = []
    if not np.array_equal(dmax.view(np.int32), ref.dmax.astype(np.float32).view(np.int32)):
        failed.append(f"dmax {dmax.tolist()} is not the per-image max {ref.dmax.tolist()}")
    _check_render(failed, "x".join(map(str, shape)) + (f" {variant}" if variant else ""), dtype, x4, gt, ref)
    assert not failed, "\n".join(failed)
    return dens, dmax


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", R.RENDER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_synth_render_elementwise(ext, shape, dtype):
    """gt within 2 * 64 u sum|v|, dmax bit for bit (the pre-fill of NaN bits shows the memset), the image within half a
    16-bit ulp + A_IMAGE / std_c, channel 3 the word 0.  16 x 16: the noise grid is 1 x 1 and every tap clamps."""
    _render_case(ext, shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["scaled", "zero0"])
def test_synth_render_per_image_dmax(ext, variant, dtype):
    """Image 1 a hundred times image 0's scale, and image 0 all zero (dmax = +0, the blob 0 * 1e6 = 0)."""
    dens, dmax = _render_case(ext, (2, 32, 48), dtype, variant)
    assert dmax[1] > 10 * dmax[0]
    if variant == "zero0":
        assert dmax.view(np.int32)[0] == 0


def test_synth_render_second_grid_sweeps(ext):
    """2048 x 2064: 66048 gt cells (more than the 256 blocks of 256 threads of the capped grid) and 4.2 M pixels (more
    than 1024 blocks of 256): the first kernel takes a ragged second sweep, the second seventeen, the last ragged."""
    n, H, W = R.RENDER_LARGE
    assert (H // 8) * (W // 8) > 256 * 256 and H * W > 1024 * 256 and (H * W) % (1024 * 256)
    _render_case(ext, R.RENDER_LARGE, torch.bfloat16)


@pytest.mark.parametrize("n,H,W", [(1, 24, 16), (1, 16, 24), (0, 16, 16)], ids=["H=24", "W=24", "n=0"])
def test_synth_render_refusals_write_nothing(ext, n, H, W):
    C, X = ext
    dens, nz = torch.rand(2, 32, 32, device="cuda"), torch.rand(2, 3, 2, 2, device="cuda")
    x4, gt, dmax = _full((2, 32, 32, 4), -1, torch.int16), _full((2, 4, 4), NAN), _full((2,), NAN)
    with pytest.raises(RuntimeError, match="synth_render"):
        C.synth_render(dens.data_ptr(), nz.data_ptr(), dmax.data_ptr(), x4.data_ptr(), gt.data_ptr(), n, H, W,
                       _dt(torch.bfloat16), X.stream_ptr())
    torch.cuda.synchronize()
    assert bool((x4 == -1).all()) and bool(torch.isnan(gt).all()) and bool(torch.isnan(dmax).all())


# ------------------------------------------------------------------------------------------- generator end to end
@functools.lru_cache(maxsize=None)
def _synthetic_ref(seed, h, w, heads):
    """Computed once per (seed, shape) and shared; nothing changes it."""
    ref, sp = R.synthetic_ref(seed, h, w, heads)
    b = sp.bound()
    # the splat's error through the blob 0.3 d / (dmax + 1e-6): the pixel's own bound, and the bound of the pixel that
    # holds the max (|max a - max b| <= max |a - b|) times d / dmax <= 1, both over std_c
    std = np.array(R.IMAGENET_STD).reshape(1, 3, 1, 1)
    extra_img = 0.3 * (b + b.max())[None, None] / (float(ref.dmax[0]) + 1e-6) / std
    extra_gt = b.reshape(1, h // 8, 8, w // 8, 8).sum(axis=(2, 4))
    return ref, extra_img, extra_gt


def _check_generated(failed, case, dtype, x4, gt, seed, h, w, heads):
    ref, extra_img, extra_gt = _synthetic_ref(seed, h, w, heads)
    _check_render(failed, case, dtype, x4.view(torch.int16).cpu().numpy(), gt[:, 0].cpu().numpy(), ref, extra_img,
                  extra_gt)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("h,w,seed,heads", [R.SYNTH_CASES[0], R.SYNTH_CASES[2]])
def test_generator_is_the_cpu_recipe(h, w, seed, heads, dtype):
    """make_synthetic_batch_gpu(1, ...) against render_ref(splat_ref(points, 4.0), noise), the points and the noise
    redrawn from the seed (the reference test_density_reference_cpu.py holds to make_synthetic_batch(1, ...)): gt within
    the pooled splat bound + the pool bound, the image within half a 16-bit ulp + A_IMAGE / std_c + the splat bound
    through 0.3 / (dmax + 1e-6) / std_c."""
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch_gpu
    x4, gt = make_synthetic_batch_gpu(1, h, w, seed=seed, heads=heads, dtype=dtype)
    torch.cuda.synchronize()
    failed = []
    _check_generated(failed, f"generator {h}x{w} seed {seed}", dtype, x4, gt, seed, h, w, heads)
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_generator_per_image_seeds(dtype):
    """seeds=[a, b, c] in one call: image i is, within the same bounds, the reference for seeds[i] alone."""
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch_gpu
    h, w, _, heads = R.SYNTH_CASES[2]
    seeds = [2, 11, 12]
    x4, gt = make_synthetic_batch_gpu(3, h, w, seeds=seeds, heads=heads, dtype=dtype)
    torch.cuda.synchronize()
    failed = []
    for i, sd in enumerate(seeds):
        _check_generated(failed, f"generator seeds[{i}]={sd}", dtype, x4[i:i + 1], gt[i:i + 1], sd, h, w, heads)
    assert not failed, "\n".join(failed)
