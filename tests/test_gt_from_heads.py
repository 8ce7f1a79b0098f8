"""Ground truth from head records on the CPU: heads_table, heads_to_gt and its padded form against the fp64 oracle of
tests/gt_heads_reference.py (D from the definition, Oy D Ox^T), the shipped generator, the dataset and the collate.
The GPU kernel is held to the same oracle in tests/test_gpu_gt_from_heads.py."""
import os

import numpy as np
import pytest
import torch

import gt_heads_reference as G
from can_distributed_pytorch_amd.data import dataset as DS
from can_distributed_pytorch_amd.data.dataset import CrowdDataset, crop_draw, crop_window, scale_draw, scaled_window
from can_distributed_pytorch_amd.data.density import (gaussian_filter_density, generate_dataset_density, heads_path,
                                                      heads_table, knn_sigmas)
from can_distributed_pytorch_amd.data.transforms import heads_to_gt, heads_to_gt64, heads_to_gt_padded
from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, _unpack

H0, W0 = 70, 100
# (window, ch, cw): sh / ch of 4, 2, 1, 0.75, 0.25, an anisotropic window and one with odd, non-dividing extents
WINDOWS = [((3, 2, 64, 96), 16, 24), ((20, 30, 32, 48), 16, 24), ((54, 76, 16, 24), 16, 24), ((5, 7, 12, 18), 16, 24),
           ((33, 41, 4, 6), 16, 24), ((0, 0, 70, 25), 32, 40), ((1, 3, 37, 53), 32, 40)]


def _heads(window):
    return np.concatenate([G.edge_heads(H0, W0, window), G.mixed_heads(H0, W0, 40, seed=sum(window))])


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("window,ch,cw", WINDOWS)
def test_definition_against_the_oracle(window, ch, cw, flip):
    """heads_to_gt == Oy D Ox^T to 1e-12 relative (of the largest cell; the fp32 output rounding apart, so the fp64
    value before it is compared), and its sum == the window's density mass to 1e-12."""
    heads = _heads(window)
    D = G.density_from_heads(heads, H0, W0)
    want = G.gt_oracle(heads, H0, W0, window, ch // 8, cw // 8, flip, D)
    got = heads_to_gt(heads, H0, W0, window, ch, cw, 8, flip)
    assert got.shape == (1, ch // 8, cw // 8) and got.dtype == np.float32
    acc = heads_to_gt64(heads, H0, W0, window, ch, cw, 8, flip)         # the value before the float32 rounding
    assert np.array_equal(got[0], acc.astype(np.float32))
    assert np.abs(acc - want).max() <= 1e-12 * np.abs(want).max()
    y0, x0, sh, sw = window
    mass = D[y0:y0 + sh, x0:x0 + sw].sum()
    assert abs(acc.sum() - mass) <= 1e-12 * mass
    assert abs(float(got.astype(np.float64).sum()) - mass) <= got.size * 2.0 ** -24 * mass


def test_sanity_against_the_shipped_generator():
    """For records made by heads_table from points, D agrees with gaussian_filter_density: the float32 sigma is the only
    difference, (2a + 2) 2^-24 relative per head term (a the Gaussian exponent: d/dsigma of exp(-a) / norm), plus the
    function's float32 output rounding."""
    rng = np.random.default_rng(3)
    pts = np.stack([rng.random(60) * (W0 + 6) - 3, rng.random(60) * (H0 + 6) - 3], 1)
    heads = heads_table(pts, (H0, W0))
    ref = gaussian_filter_density((H0, W0), pts).astype(np.float64)
    D = G.density_from_heads(heads, H0, W0)
    bound = np.zeros((H0, W0))
    for c, r, s, R in heads.astype(np.float64):
        k, R = G.kernel1d(s, R)
        ys, xs = np.arange(H0) - r, np.arange(W0) - c
        ky = np.where(np.abs(ys) <= R, k[np.clip(ys + R, 0, 2 * R).astype(int)], 0.0)
        kx = np.where(np.abs(xs) <= R, k[np.clip(xs + R, 0, 2 * R).astype(int)], 0.0)
        a = (ys[:, None] ** 2 + xs[None, :] ** 2) / (2.0 * s * s) if s > 0 else np.zeros((H0, W0))
        bound += np.outer(ky, kx) * (2.0 * a + 2.0) * 2.0 ** -24
    assert np.all(np.abs(D - ref) <= bound + 2.0 ** -24 * ref)
    assert D.sum() > 30


def test_heads_table_records():
    """Out-of-image heads are skipped (they still count as neighbours), c, r = int(x), int(y), sigma the float32 of the
    float64 knn sigma, R = int(4 sigma64 + 0.5) from the FLOAT64 sigma; coincident heads are deltas with R = 0."""
    pts = np.array([[10.7, 5.2], [-0.5, 3.0], [99.9, 69.9], [100.0, 10.0], [50.0, 70.0], [30.2, 40.9], [31.0, 44.0]])
    sig = knn_sigmas(pts, (H0, W0))
    t = heads_table(pts, (H0, W0))
    keep = [0, 2, 5, 6]
    assert t.dtype == np.float32 and t.shape == (4, 4)
    assert t[:, 0].tolist() == [10, 99, 30, 31] and t[:, 1].tolist() == [5, 69, 40, 44]
    assert np.array_equal(t[:, 2], sig[keep].astype(np.float32))
    assert t[:, 3].tolist() == [int(4.0 * s + 0.5) for s in sig[keep]]
    # a sigma whose float32 rounding crosses the radius step: 4 s + 0.5 just below an integer in float64 only
    s64 = np.nextafter(2.125, 0.0)
    assert int(4.0 * s64 + 0.5) == 8 and int(4.0 * float(np.float32(s64)) + 0.5) == 9
    d = s64 / 0.2                                                # two heads: sigma = 0.1 * (d + d)... one neighbour
    two = heads_table(np.array([[20.0, 20.0], [20.0 + d, 20.0]]), (H0, W0))
    s_two = knn_sigmas(np.array([[20.0, 20.0], [20.0 + d, 20.0]]), (H0, W0))
    assert two[:, 3].tolist() == [int(4.0 * s + 0.5) for s in s_two]
    same = heads_table(np.tile([[10.5, 7.25]], (4, 1)), (H0, W0))
    assert same[:, 2:].tolist() == [[0.0, 0.0]] * 4
    assert heads_table(np.zeros((0, 2)), (H0, W0)).shape == (0, 4)
    one = heads_table(np.array([[5.0, 6.0]]), (H0, W0))
    assert one.tolist() == [[5.0, 6.0, (H0 + W0) / 8.0, int((H0 + W0) / 2.0 + 0.5)]]       # one head: avg(shape) / 4


@pytest.mark.parametrize("flip", [False, True])
def test_unscaled_window_is_box_sums(flip):
    """sh = ch, sw = cw: every cell is the d x d box sum of D; the padded form on an image smaller than the crop has
    box sums in the valid cells and 0 in the rest."""
    window = (54, 76, 16, 24)
    heads = _heads(window)
    D = G.density_from_heads(heads, H0, W0)
    got = heads_to_gt(heads, H0, W0, window, 16, 24, 8, flip)[0]
    want = G.box_sums(D, 54, 76, 16, 24, 8, flip)
    assert np.abs(got - want).max() <= 2.0 ** -24 * want.max()
    assert np.array_equal(heads_to_gt_padded(heads, H0, W0, 54, 76, 16, 24, 8, flip)[0], got)
    h0, w0 = 20, 30                                              # smaller than the 32 x 40 crop: valid 16 x 24
    small = np.concatenate([G.edge_heads(h0, w0, (2, 3, 16, 24)), G.mixed_heads(h0, w0, 20, seed=5)])
    Ds = G.density_from_heads(small, h0, w0)
    assert crop_window(h0, w0, 32, 40, 8) == (16, 24)
    pad = heads_to_gt_padded(small, h0, w0, 2, 3, 32, 40, 8, flip)
    assert pad.shape == (1, 4, 5) and pad.dtype == np.float32
    want = G.box_sums(Ds, 2, 3, 16, 24, 8, flip)
    assert np.abs(pad[0, :2, :3] - want).max() <= 2.0 ** -24 * want.max()
    assert not pad[0, 2:].any() and not pad[0, :, 3:].any()


def test_heads_outside_the_window_add_nothing_and_bad_windows_raise():
    far = np.asarray([G.record(5, 5, 2.0), G.record(95, 65, 0.0)], dtype=np.float32)
    assert not heads_to_gt(far, H0, W0, (30, 40, 16, 24), 16, 24, 8, False).any()
    assert not heads_to_gt(np.zeros((0, 4), np.float32), H0, W0, (30, 40, 16, 24), 16, 24, 8, False).any()
    for window in [(60, 0, 16, 24), (0, 80, 16, 24), (-1, 0, 16, 24), (0, 0, 0, 24)]:
        with pytest.raises(ValueError, match="window"):
            heads_to_gt(far, H0, W0, window, 16, 24, 8, False)
    with pytest.raises(ValueError, match="multiple"):
        heads_to_gt(far, H0, W0, (0, 0, 16, 24), 16, 20, 8, False)


# --------------------------------------------------------------------------------------------------- dataset, collate
SIZES = [(40, 56), (20, 30), (90, 150)]


@pytest.fixture(scope="module")
def tiny_root(tmp_path_factory):
    """Three PNG images of mixed size with maps and head sidecars; (img_root, gt_root, points per image)."""
    from PIL import Image
    root = tmp_path_factory.mktemp("heads_ds")
    img_root, gt_root = root / "images", root / "ground_truth"
    img_root.mkdir(), gt_root.mkdir()
    rng = np.random.default_rng(11)
    pts = {}
    for k, (h, w) in enumerate(SIZES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(img_root / f"IMG_{k}.png")
        p = np.stack([rng.random(12 + 9 * k) * w, rng.random(12 + 9 * k) * h], 1)
        pts[f"IMG_{k}.png"] = p
        np.save(gt_root / f"IMG_{k}.npy", gaussian_filter_density((h, w), p))
        np.save(heads_path(str(gt_root / f"IMG_{k}.npy")), heads_table(p, (h, w)))
    return str(img_root), str(gt_root), pts


@pytest.mark.parametrize("scale", [None, (0.5, 2.0)])
def test_dataset_items(tiny_root, scale):
    """raw=False: the images of the map-based item bit for bit, every ground truth heads_to_gt / heads_to_gt_padded of
    the drawn window.  raw=True: (the same uint8 image, the head table, the same windows)."""
    img_root, gt_root, pts = tiny_root
    kw = dict(gt_downsample=8, phase="train", seed=3, crop=(32, 40), crops_per_image=3, crop_scale=scale)
    old = CrowdDataset(img_root, gt_root, **kw)
    new = CrowdDataset(img_root, gt_root, gt_from_heads=True, **kw)
    old_raw = CrowdDataset(img_root, gt_root, raw=True, **kw)
    new_raw = CrowdDataset(img_root, gt_root, raw=True, gt_from_heads=True, **kw)
    for i, (h0, w0) in enumerate(SIZES):
        name = f"IMG_{i}.png"
        heads = heads_table(pts[name], (h0, w0))
        im_o, gt_o = old[(i, 2)]
        im_n, gt_n = new[(i, 2)]
        assert torch.equal(im_o, im_n) and gt_n.shape == gt_o.shape and gt_n.dtype == torch.float32
        img_r, tab, win = new_raw[(i, 2)]
        img_o, _, win_o = old_raw[(i, 2)]
        assert torch.equal(img_r, img_o) and torch.equal(win, win_o)
        assert tab.dtype == torch.float32 and np.array_equal(tab.numpy(), heads)
        for k in range(3):
            if scale is None:
                wh, ww = crop_window(h0, w0, 32, 40, 8)
            else:
                wh, ww = scaled_window(h0, w0, 32, 40, scale_draw(3, 2, i, k, *scale))
            y0, x0, fl = crop_draw(3, 2, i, k, h0 - wh + 1, w0 - ww + 1)
            assert win[k].tolist() == [y0, x0, int(fl)] + ([wh, ww] if scale else [])
            want = heads_to_gt(heads, h0, w0, (y0, x0, wh, ww), 32, 40, 8, fl) if scale else \
                heads_to_gt_padded(heads, h0, w0, y0, x0, 32, 40, 8, fl)
            assert np.array_equal(gt_n[k].numpy(), want)
            D = G.density_from_heads(heads, h0, w0)
            if wh and ww:
                mass = D[y0:y0 + wh, x0:x0 + ww].sum()
                assert abs(float(gt_n[k].double().sum()) - mass) <= 1e-5 * mass + 1e-12


def test_draws_are_what_they_were():
    # the draws hash (seed, epoch, index, k) alone: pinned values of the chain, computed from its definition
    s = DS._draw_state(7, 5, 11, 2)
    assert crop_draw(7, 5, 11, 2, 50, 60) == (int((DS._splitmix64(s ^ 1) * 50) >> 64), int((DS._splitmix64(s ^ 2) * 60) >> 64),
                                              bool(DS._splitmix64(s ^ 3) >> 63))
    u = (DS._splitmix64(s ^ 4) >> 11) / 2 ** 53
    assert scale_draw(7, 5, 11, 2, 0.5, 2.0) == float(min(2.0, max(0.5, 0.5 * 4.0 ** u)))


def test_missing_sidecar_and_missing_crop_raise(tiny_root, tmp_path):
    img_root, gt_root, _ = tiny_root
    with pytest.raises(ValueError, match="crop"):
        CrowdDataset(img_root, gt_root, gt_downsample=8, gt_from_heads=True)
    with pytest.raises(ValueError, match="crop"):
        PackedCollate(gt_from_heads=True)
    empty = tmp_path / "gt"
    empty.mkdir()
    ds = CrowdDataset(img_root, str(empty), gt_downsample=8, crop=(32, 40), gt_from_heads=True)
    with pytest.raises(ValueError, match="--heads"):
        ds[0]


@pytest.mark.parametrize("scale", [None, (0.5, 2.0)])
def test_collate_packs_k_crops_against_one_head_range(tiny_root, scale):
    """The heads pack: the image bytes and descriptors of the map-based pack of the same windows, a zero ground truth
    region, one (first head, count) range per output sample shared by an image's K crops, the head table, and a meta
    tuple of eight fields; packs of the existing kinds are byte for byte what the collate makes with the option off."""
    img_root, gt_root, pts = tiny_root
    kw = dict(gt_downsample=8, phase="train", seed=3, raw=True, crop=(32, 40), crops_per_image=3, crop_scale=scale)
    old = CrowdDataset(img_root, gt_root, **kw)
    new = CrowdDataset(img_root, gt_root, gt_from_heads=True, **kw)
    items_old, items_new = [old[(i, 1)] for i in range(3)], [new[(i, 1)] for i in range(3)]
    b_old, m_old = PackedCollate(crop=(32, 40), crop_scale=scale is not None)(items_old)
    b_off, m_off = PackedCollate(crop=(32, 40), crop_scale=scale is not None, gt_from_heads=False)(items_old)
    ioff = sum(h * w * 3 for h, w in SIZES)                      # (the alignment gap behind the images is not written)
    assert m_old == m_off and len(m_old) == (7 if scale else 6)
    assert torch.equal(b_old[:ioff], b_off[:ioff]) and torch.equal(b_old[m_old[3]:], b_off[m_old[3]:])
    buf, meta = PackedCollate(crop=(32, 40), crop_scale=scale is not None, gt_from_heads=True)(items_new)
    n, ho, wo, goff, doff = meta[:5]
    counts = [len(heads_table(pts[f"IMG_{i}.png"], SIZES[i])) for i in range(3)]
    assert len(meta) == 8 and meta[:5] == m_old[:5] and meta[5:] == (3, int(scale is not None), sum(counts))
    assert n == 9 and buf.numel() == doff + 64 * n + 16 * n + 16 * sum(counts)
    assert torch.equal(buf[:ioff], b_old[:ioff]) and torch.equal(buf[doff:doff + 64 * n], b_old[doff:])
    assert not buf[goff:doff].any()
    ranges = buf[doff + 64 * n:doff + 80 * n].view(torch.int64).view(n, 2).tolist()
    starts = [0, counts[0], counts[0] + counts[1]]
    assert ranges == [[starts[i // 3], counts[i // 3]] for i in range(9)]
    table = buf[doff + 80 * n:].view(torch.float32).view(-1, 4).numpy()
    assert np.array_equal(table, np.concatenate([heads_table(pts[f"IMG_{i}.png"], SIZES[i]) for i in range(3)]))
    _, dims, kind = _unpack((buf, meta))
    assert dims == (n, ho, wo, goff, doff) and kind == ("crop_scaled+heads" if scale else "crop+heads")
    assert _unpack((b_old, m_old))[2] == ("crop_scaled" if scale else "crop")
    with pytest.raises(ValueError):
        _unpack((buf[:-16], meta))
    with pytest.raises(ValueError):
        _unpack((buf, meta[:7] + (meta[7] + 1,)))
    with pytest.raises(ValueError, match="head records"):
        PackedCollate(crop=(32, 40), crop_scale=scale is not None, gt_from_heads=True)(items_old)


def test_driver_writes_sidecars_only_with_heads(tmp_path, monkeypatch):
    """generate_dataset_density(heads=True) writes IMG_k.heads.npy and nothing else; without it, the map alone."""
    from PIL import Image
    from can_distributed_pytorch_amd.data import density as DN
    part = tmp_path / "train_data"
    (part / "images").mkdir(parents=True), (part / "ground_truth").mkdir()
    Image.fromarray(np.zeros((24, 32, 3), np.uint8)).save(part / "images" / "IMG_1.jpg")
    pts = np.array([[3.5, 4.5], [20.0, 10.0], [31.9, 23.9], [40.0, 2.0]])
    monkeypatch.setattr(DN, "load_sha_points", lambda mat: pts)
    assert generate_dataset_density(str(tmp_path), parts=("train_data",)) == 1
    assert sorted(os.listdir(part / "ground_truth")) == ["IMG_1.npy"]
    assert generate_dataset_density(str(tmp_path), parts=("train_data",), heads=True) == 1
    assert sorted(os.listdir(part / "ground_truth")) == ["IMG_1.heads.npy", "IMG_1.npy"]
    assert np.array_equal(np.load(part / "ground_truth" / "IMG_1.heads.npy"), heads_table(pts, (24, 32)))
    assert np.array_equal(np.load(part / "ground_truth" / "IMG_1.npy"), gaussian_filter_density((24, 32), pts))


def test_train_flag_needs_crop_size():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "train_cli", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    assert p.parse_args([]).gt_from_heads is False
    assert p.parse_args(["--crop-size", "32x40", "--gt-from-heads"]).gt_from_heads is True
    with pytest.raises(SystemExit):
        p.parse_args(["--gt-from-heads"])
