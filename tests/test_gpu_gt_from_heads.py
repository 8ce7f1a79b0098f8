"""csrc/density.hip:gt_from_heads_kernel through its raw entry C.gt_from_heads, and the heads pack through
preprocess_packed / AheadPrep, against the fp64 definition of tests/gt_heads_reference.py.

Per cell the kernel is held to (u = 2^-24, the project's error model for __expf terms, README round 15)

  u [ sum_h c_h (20 (1 + A_y,h + A_x,h) + n_y,h + n_x,h + 2) + (n_h - 1) sum_h c_h ]

with c_h head h's fp64 contribution to the cell, A the largest exponents among the terms of its two profile entries,
n_y, n_x their numbers of terms and n_h the heads whose footprint reaches the cell; a cell no footprint reaches must be
+0 bits.  The output is pre-filled with NaN (every cell must be written), two launches must agree bit for bit, and the
worst err / bound per case is printed with ``pytest -s`` (profiles/r16/gt_from_heads_errors.txt).  The kernel stages
256 heads at once: 700 heads are three chunks, the last ragged.
"""
import functools

import numpy as np
import pytest
import torch

import gt_heads_reference as G

pytestmark = pytest.mark.gpu

NAN = float("nan")
D8 = 8
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for case, r in _worst.items():
        print(f"\nGT_FROM_HEADS {case:<34s} worst err/bound {r:.4f}", end="")
    if _worst:
        print(f"\nGT_FROM_HEADS worst err / bound over all cases: {max(_worst.values()):.4f}")


@pytest.fixture(scope="module")
def ext():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require(), _ext


def _desc(samples, H0, W0):
    """[n, 8] int64 descriptors: sample = (y0, x0, flip) unscaled or (y0, x0, flip, sh, sw); no image bytes."""
    return torch.tensor([[0, H0, W0, 3, int(s[2]), s[0], s[1], 1 if len(s) == 3 else (s[3] << 32) | s[4]]
                         for s in samples], dtype=torch.int64)


def _render(ext, heads, ranges, desc, ch, cw, fill=NAN):
    """One C.gt_from_heads call on host tensors (heads [N, 4] fp32, ranges [n, 2] and desc [n, 8] int64), the output
    pre-filled: fp32 numpy [n, ch/8, cw/8]."""
    C, X = ext
    heads = torch.from_numpy(np.ascontiguousarray(heads, dtype=np.float32).reshape(-1, 4))
    ranges = torch.as_tensor(ranges, dtype=torch.int64).reshape(-1, 2).contiguous()
    n = desc.shape[0]
    hd, rd, dd = heads.cuda(), ranges.cuda(), desc.cuda()
    gt = torch.full((n, 1, ch // D8, cw // D8), fill, dtype=torch.float32, device="cuda")
    C.gt_from_heads(hd.data_ptr(), rd.data_ptr(), dd.data_ptr(), heads.data_ptr(), heads.shape[0], ranges.data_ptr(),
                    desc.data_ptr(), n, gt.data_ptr(), ch, cw, D8, X.stream_ptr())
    torch.cuda.synchronize()
    return gt[:, 0].cpu().numpy()


def _check(failed, case, out, terms):
    """out [rows, cols] against the fp64 terms: within the bound, +0 bits where no footprint reaches."""
    if np.isnan(out).any():
        failed.append(f"{case}: a cell was not written")
        return
    if out.view(np.int32)[terms.reached == 0].any():
        failed.append(f"{case}: a cell no footprint reaches is not +0")
    ratio = G.worst_ratio(np.abs(out.astype(np.float64) - terms.value), terms.bound)
    _worst[case] = max(_worst.get(case, 0.0), ratio)
    if not ratio <= 1.0:
        failed.append(f"{case}: err / bound = {ratio:.4g}")


def _terms(heads, H0, W0, s, ch, cw):
    if len(s) == 3:
        return G.padded_terms(heads, H0, W0, s[0], s[1], ch, cw, D8, bool(s[2]))
    return G.gt_terms(heads, H0, W0, (s[0], s[1], s[3], s[4]), ch // D8, cw // D8, bool(s[2]))


# (H0, W0, ch, cw, [(y0, x0, flip, sh, sw) ...]): sh / ch of 4, 2, 1, 0.75, 0.25, anisotropic windows, both flips; the
# last case has 17 x 33 cells, 2 x 3 tiles of 16 x 16 with ragged edges
SCALED = {
    "16x24 in 70x100": (70, 100, 16, 24, [(3, 2, 0, 64, 96), (20, 30, 1, 32, 48), (54, 76, 0, 16, 24),
                                          (5, 7, 1, 12, 18), (33, 41, 0, 4, 6), (66, 94, 1, 4, 6)]),
    "32x40 in 90x150": (90, 150, 32, 40, [(10, 20, 1, 64, 80), (58, 110, 0, 32, 40), (0, 0, 1, 24, 30),
                                          (41, 77, 0, 8, 10), (1, 3, 0, 37, 53), (0, 0, 1, 90, 150)]),
    "32x40 in 20x150": (20, 150, 32, 40, [(0, 45, 0, 20, 60), (0, 90, 1, 20, 25)]),
    "64x128 in 90x150": (90, 150, 64, 128, [(13, 11, 0, 64, 128), (42, 54, 1, 48, 96), (60, 100, 0, 16, 32),
                                            (0, 0, 1, 90, 150)]),
    "136x264 in 90x150": (90, 150, 136, 264, [(11, 9, 1, 68, 132), (0, 0, 0, 90, 150), (30, 60, 1, 34, 66)]),
}
COUNTS = [0, 1, 5, 700]


@functools.lru_cache(maxsize=None)
def _case_heads(name, count):
    """The records of a case: 0; the single head of the reference (sigma (H + W) / 8: R larger than the image); the
    first five edge heads of the first window; or the edge heads of the first window (sigmas 0.6, 2, 4, a delta and
    sigma 30 with R = 120, on the window's first and last row and column, cut by the window and by the image) followed by
    random heads up to `count`."""
    H0, W0, _, _, samples = SCALED[name]
    s = samples[0]
    if count == 0:
        return np.zeros((0, 4), dtype=np.float32)
    if count == 1:
        return np.asarray([G.record(W0 // 3, H0 // 2, (H0 + W0) / 8.0)], dtype=np.float32)
    edge = G.edge_heads(H0, W0, (s[0], s[1], s[3], s[4]))
    if count <= len(edge):
        return edge[[0, 1, 3, 8, 9]][:count]
    return np.concatenate([edge, G.mixed_heads(H0, W0, count - len(edge), seed=count)])


@functools.lru_cache(maxsize=None)
def _case_terms(name, count):
    """Computed once per case and shared; nothing changes it."""
    H0, W0, ch, cw, samples = SCALED[name]
    return [_terms(_case_heads(name, count), H0, W0, s, ch, cw) for s in samples]


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", list(SCALED))
def test_scaled_windows_within_the_bound(ext, name, count):
    H0, W0, ch, cw, samples = SCALED[name]
    heads = _case_heads(name, count)
    desc = _desc(samples, H0, W0)
    ranges = [[0, len(heads)]] * len(samples)
    out = _render(ext, heads, ranges, desc, ch, cw)
    failed = []
    for i, t in enumerate(_case_terms(name, count)):
        _check(failed, f"{name} n={count} s{i}", out[i], t)
    if count == 0:
        assert not out.view(np.int32).any()
    again = _render(ext, heads, ranges, desc, ch, cw, fill=7.0)
    assert np.array_equal(out.view(np.int32), again.view(np.int32)), "two launches differ"
    assert not failed, "\n".join(failed)


def test_unscaled_windows_are_box_sums(ext):
    """The unscaled marker: crops inside a larger image, and the padded crop of an image smaller than the 32 x 40 crop
    (valid 16 x 24: box sums there, +0 in the padding), against the fp64 box sums within the same bound."""
    failed = []
    for H0, W0, samples in [(90, 150, [(0, 0, 0), (58, 110, 1), (17, 33, 0)]), (20, 30, [(2, 3, 0), (4, 6, 1), (0, 0, 1)]),
                            (35, 30, [(3, 1, 1)]), (7, 150, [(0, 5, 0)])]:
        heads = np.concatenate([G.edge_heads(H0, W0, (samples[0][0], samples[0][1], min(32, H0 // 8 * 8) or 1,
                                                      min(40, W0 // 8 * 8))), G.mixed_heads(H0, W0, 300, seed=H0)])
        out = _render(ext, heads, [[0, len(heads)]] * len(samples), _desc(samples, H0, W0), 32, 40)
        D = G.density_from_heads(heads, H0, W0)
        vh, vw = min(32, H0 // 8 * 8), min(40, W0 // 8 * 8)
        for i, s in enumerate(samples):
            t = _terms(heads, H0, W0, s, 32, 40)
            _check(failed, f"unscaled 32x40 in {H0}x{W0} s{i}", out[i], t)
            if vh and vw:
                box = G.box_sums(D, s[0], s[1], vh, vw, 8, bool(s[2]))
                assert np.abs(t.value[:vh // 8, :vw // 8] - box).max() <= 1e-12 * box.max()      # the oracle itself
            assert not out[i, vh // 8:].view(np.int32).any() and not out[i, :, vw // 8:].view(np.int32).any()
    assert not failed, "\n".join(failed)


def test_batch_of_two_images_k3(ext):
    """Two images of different size and head count, one of them without heads, K = 3 crops each against the image's one
    range; the second image's range starts behind the first's records."""
    ch, cw = 32, 40
    a = np.concatenate([G.edge_heads(90, 150, (10, 20, 64, 80)), G.mixed_heads(90, 150, 290, seed=1)])
    b = G.mixed_heads(40, 56, 37, seed=2)
    sa = [(10, 20, 1, 64, 80), (58, 110, 0, 32, 40), (0, 0, 1, 24, 30)]
    sb = [(0, 0, 0, 40, 56), (8, 16, 1, 32, 40), (3, 5, 0, 16, 20)]
    failed = []
    for first, second, hf, hs in [(a, np.zeros((0, 4), np.float32), (90, 150), (40, 56)),
                                  (np.zeros((0, 4), np.float32), b, (90, 150), (40, 56)), (a, b, (90, 150), (40, 56))]:
        heads = np.concatenate([first, second])
        desc = torch.cat([_desc(sa, *hf), _desc(sb, *hs)])
        ranges = [[0, len(first)]] * 3 + [[len(first), len(second)]] * 3
        out = _render(ext, heads, ranges, desc, ch, cw)
        for i in range(3):
            _check(failed, f"batch {len(first)}+{len(second)} a{i}", out[i], _terms(first, *hf, sa[i], ch, cw))
            _check(failed, f"batch {len(first)}+{len(second)} b{i}", out[3 + i], _terms(second, *hs, sb[i], ch, cw))
    assert not failed, "\n".join(failed)


def test_host_check_refuses_without_launching(ext):
    """A window that leaves its image, a head range that leaves the table, a negative or non-integer R, a non-finite
    sigma, a crop that is no multiple of d (and a head outside its image): an error code from the host check, a
    RuntimeError from the entry, and the output untouched."""
    C, X = ext
    H0, W0, ch, cw = 70, 100, 16, 24
    good_heads = np.asarray([G.record(10, 10, 2.0), G.record(50, 30, 4.0)], dtype=np.float32)
    good_desc = _desc([(3, 2, 0, 64, 96), (54, 76, 1)], H0, W0)
    good_ranges = [[0, 2], [0, 2]]

    def run(heads=good_heads, ranges=good_ranges, desc=good_desc, ch=ch, cw=cw):
        h = torch.from_numpy(np.ascontiguousarray(heads, dtype=np.float32).reshape(-1, 4))
        r = torch.tensor(ranges, dtype=torch.int64)
        code = C.gt_from_heads_check(h.data_ptr(), h.shape[0], r.data_ptr(), desc.data_ptr(), desc.shape[0], ch, cw, D8)
        hd, rd, dd = h.cuda(), r.cuda(), desc.cuda()
        gt = torch.full((desc.shape[0], 1, 2, 3), 7.0, device="cuda")
        try:
            C.gt_from_heads(hd.data_ptr(), rd.data_ptr(), dd.data_ptr(), h.data_ptr(), h.shape[0], r.data_ptr(),
                            desc.data_ptr(), desc.shape[0], gt.data_ptr(), ch, cw, D8, X.stream_ptr())
            raised = False
        except RuntimeError as e:
            raised = "gt_from_heads" in str(e)
        torch.cuda.synchronize()
        return code, raised, bool((gt == 7.0).all())

    assert run() == (0, False, False)

    def heads_with(col, value):
        h = good_heads.copy()
        h[1, col] = value
        return h

    bad = {
        "window below": dict(desc=_desc([(7, 2, 0, 64, 96)], H0, W0), ranges=[[0, 2]]),
        "window right": dict(desc=_desc([(3, 5, 0, 64, 96)], H0, W0), ranges=[[0, 2]]),
        "window negative": dict(desc=_desc([(-1, 2, 0, 16, 24)], H0, W0), ranges=[[0, 2]]),
        "window empty": dict(desc=_desc([(3, 2, 0, 0, 24)], H0, W0), ranges=[[0, 2]]),
        "unscaled window leaves": dict(desc=_desc([(55, 76, 1)], H0, W0), ranges=[[0, 2]]),
        "range past the table": dict(ranges=[[0, 2], [1, 2]]),
        "range negative": dict(ranges=[[-1, 2], [0, 2]]),
        "count negative": dict(ranges=[[0, 2], [0, -1]]),
        "R negative": dict(heads=heads_with(3, -1.0)),
        "R not an integer": dict(heads=heads_with(3, 16.5)),
        "R NaN": dict(heads=heads_with(3, NAN)),
        "sigma inf": dict(heads=heads_with(2, float("inf"))),
        "sigma NaN": dict(heads=heads_with(2, NAN)),
        "head outside its image": dict(heads=heads_with(0, 100.0)),
        "crop no multiple of d": dict(cw=20),
    }
    for name, kw in bad.items():
        code, raised, untouched = run(**kw)
        assert code != 0 and raised and untouched, (name, code, raised, untouched)


# ------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def tiny_root(tmp_path_factory):
    from PIL import Image
    from can_distributed_pytorch_amd.data.density import gaussian_filter_density, heads_path, heads_table
    root = tmp_path_factory.mktemp("heads_ds_gpu")
    img_root, gt_root = root / "images", root / "ground_truth"
    img_root.mkdir(), gt_root.mkdir()
    rng = np.random.default_rng(11)
    tables = []
    for k, (h, w) in enumerate([(40, 56), (20, 30), (90, 150)]):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(img_root / f"IMG_{k}.png")
        p = np.stack([rng.random(12 + 9 * k) * w, rng.random(12 + 9 * k) * h], 1)
        np.save(gt_root / f"IMG_{k}.npy", gaussian_filter_density((h, w), p))
        tables.append(((h, w), heads_table(p, (h, w))))
        np.save(heads_path(str(gt_root / f"IMG_{k}.npy")), tables[-1][1])
    return str(img_root), str(gt_root), tables


@pytest.mark.parametrize("scale", [None, (0.5, 2.0)], ids=["crop", "crop_scaled"])
def test_pipeline_end_to_end(tiny_root, scale):
    """preprocess_packed and AheadPrep.issue / ready on a heads pack: x4 bit for bit the x4 of the same windows'
    existing crop / scaled-crop pack, gt the rendered ground truth within the bound (and a view of the device buffer)."""
    from can_distributed_pytorch_amd.data.dataset import CrowdDataset
    from can_distributed_pytorch_amd.ops.preprocess import AheadPrep, PackedCollate, preprocess_packed
    img_root, gt_root, tables = tiny_root
    kw = dict(gt_downsample=8, phase="train", seed=3, raw=True, crop=(32, 40), crops_per_image=3, crop_scale=scale)
    old = CrowdDataset(img_root, gt_root, **kw)
    new = CrowdDataset(img_root, gt_root, gt_from_heads=True, **kw)
    p_old = PackedCollate(crop=(32, 40), crop_scale=scale is not None)([old[(i, 1)] for i in range(3)])
    items = [new[(i, 1)] for i in range(3)]
    p_new = PackedCollate(crop=(32, 40), crop_scale=scale is not None, gt_from_heads=True)(items)
    x_old, _ = preprocess_packed(p_old, "cuda")
    x_new, gt = preprocess_packed(p_new, "cuda")
    prep = AheadPrep("cuda")
    x_ahead, gt_ahead = prep.ready(prep.issue(p_new))
    torch.cuda.synchronize()
    assert gt.shape == (9, 1, 4, 5) and gt.dtype == torch.float32 and gt._base is not None
    assert torch.equal(x_new.view(torch.int16), x_old.view(torch.int16))
    assert torch.equal(x_ahead.view(torch.int16), x_old.view(torch.int16))
    assert torch.equal(gt.view(torch.int32), gt_ahead.view(torch.int32))
    failed = []
    out = gt[:, 0].cpu().numpy()
    for i, ((h0, w0), heads) in enumerate(tables):
        for k, w in enumerate(items[i][2].tolist()):
            _check(failed, f"pipeline {'scaled' if scale else 'crop'} img{i} k{k}", out[3 * i + k],
                   _terms(heads, h0, w0, tuple(w), 32, 40))
    assert not failed, "\n".join(failed)
    bad = (p_new[0].clone(), p_new[1])
    n, doff = p_new[1][0], p_new[1][4]
    bad[0][doff + 64 * n:doff + 64 * n + 16].view(torch.int64)[1] = 10 ** 6           # a range that leaves the table
    with pytest.raises(RuntimeError, match="gt_from_heads"):
        preprocess_packed(bad, "cuda")
    torch.cuda.synchronize()
