"""Random-scale crops on the CPU: the stateless scale draw, the source window rule, prepare_pair_scaled against
prepare_pair and against a dense-matrix float64 bilinear reference, density_to_gt_scaled, CrowdDataset(crop_scale=...),
the scaled PackedCollate layout and the train.py option."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from can_distributed_pytorch_amd.data.dataset import (CrowdDataset, EpochTaggedSampler, crop_collate, crop_draw,
                                                      density_to_gt, density_to_gt_scaled, scale_draw, scaled_window)
from can_distributed_pytorch_amd.data.transforms import (IMAGENET_MEAN, IMAGENET_STD, prepare_pair,
                                                         prepare_pair_scaled)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP = (32, 48)
D = 8
SEED = 11
SCALE = (0.5, 2.0)
SHAPES = [(20, 30), (37, 53), (64, 80), (300, 400)]


# ---------------------------------------------------------------- the draws
def test_scale_draw_is_stateless_and_in_range():
    a = [scale_draw(3, 2, 7, k, 0.75, 1.33) for k in range(4)]
    assert a == [scale_draw(3, 2, 7, k, 0.75, 1.33) for k in range(4)]
    assert a[::-1] == [scale_draw(3, 2, 7, k, 0.75, 1.33) for k in (3, 2, 1, 0)]        # any call order
    assert len(set(a)) == 4
    assert scale_draw(3, 2, 7, 0, 0.75, 1.33) not in (scale_draw(4, 2, 7, 0, 0.75, 1.33),
                                                      scale_draw(3, 3, 7, 0, 0.75, 1.33),
                                                      scale_draw(3, 2, 8, 0, 0.75, 1.33))
    draws = np.array([scale_draw(SEED, i % 7, i, i % 3, 0.75, 1.33) for i in range(10000)])
    assert draws.min() >= 0.75 and draws.max() <= 1.33
    # log-uniform: log(s) is uniform on [log lo, log hi] (mean and the halves, loosely)
    u = (np.log(draws) - math.log(0.75)) / (math.log(1.33) - math.log(0.75))
    assert abs(u.mean() - 0.5) < 0.02 and abs((u < 0.5).mean() - 0.5) < 0.02
    assert all(scale_draw(SEED, 0, i, 0, 1.25, 1.25) == 1.25 for i in range(100))
    assert all(scale_draw(SEED, 0, i, 0, 0.25, 4.0) != scale_draw(SEED, 0, i + 1, 0, 0.25, 4.0) for i in range(100))


def test_scale_draw_follows_the_documented_chain():
    from can_distributed_pytorch_amd.data.dataset import _M64, _splitmix64
    seed, epoch, index, k, lo, hi = 5, 9, 123, 2, 0.5, 2.0
    s0 = _splitmix64(_splitmix64(_splitmix64(_splitmix64(seed & _M64) ^ epoch) ^ index) ^ k)
    u = (_splitmix64(s0 ^ 4) >> 11) / 2 ** 53
    assert scale_draw(seed, epoch, index, k, lo, hi) == lo * (hi / lo) ** u


def test_crop_draw_is_what_it_was():
    """Literals computed with the code before scale_draw existed."""
    assert [crop_draw(3, 2, 7, k, 9, 9) for k in range(4)] == [(5, 8, True), (3, 2, True), (5, 7, True), (0, 6, False)]
    assert [crop_draw(11, 0, 5, k, 1000, 777) for k in range(3)] == [(181, 482, True), (559, 182, True),
                                                                     (473, 592, True)]
    assert crop_draw(2 ** 40 + 5, 123, 999, 17, 1, 1) == (0, 0, False)
    assert crop_draw(0, 0, 0, 0, 46, 54) == (29, 1, True)


def test_both_draws_are_what_they_were():
    """Literals computed with the code before the two draws shared their chain state."""
    tuples = [(3, 2, 7, 1), (11, 0, 5, 2), (2 ** 40 + 5, 123, 999, 17), (0, 0, 0, 0)]
    assert [crop_draw(*t, 1000, 777) for t in tuples] == [(436, 246, True), (473, 592, True), (697, 688, False),
                                                          (647, 15, True)]
    assert [scale_draw(*t, 0.5, 2.0) for t in tuples] == [1.485580203883466, 0.82089857378068, 1.2501406608339898,
                                                          1.4574052934975077]
    assert [scale_draw(*t, 0.75, 1.33) for t in tuples] == [1.1762222783373204, 0.9205304144750743, 1.09527443808346,
                                                            1.1669521902254036]


@pytest.mark.parametrize("h0,w0", SHAPES)
def test_window_fits_its_image(h0, w0):
    ch, cw = CROP
    for s in np.exp(np.linspace(math.log(0.25), math.log(4.0), 97)):
        sh, sw = scaled_window(h0, w0, ch, cw, float(s))
        assert 1 <= sh <= h0 and 1 <= sw <= w0
        # within the kernel's accepted range: a factor 4 either way
        assert sh <= 4 * ch and sw <= 4 * cw and ch <= 4 * sh and cw <= 4 * sw
        for i in range(20):
            y0, x0, _ = crop_draw(SEED, 1, i, 0, h0 - sh + 1, w0 - sw + 1)
            assert 0 <= y0 <= h0 - sh and 0 <= x0 <= w0 - sw
        if s > max(ch / h0, cw / w0):                          # the image allows this scale: the rounded extent
            assert (sh, sw) == (min(h0, int(math.floor(ch / s + 0.5))), min(w0, int(math.floor(cw / s + 0.5))))
    if h0 >= ch and w0 >= cw:
        assert scaled_window(h0, w0, ch, cw, 1.0) == (ch, cw)
    else:                                                      # a smaller image is upsampled: the window fills an axis
        sh, sw = scaled_window(h0, w0, ch, cw, 1.0)
        assert sh == h0 or sw == w0
    assert scaled_window(h0, w0, ch, cw, 2.0)[0] == (16 if h0 >= 16 else h0)


# ---------------------------------------------------------------- prepare_pair_scaled
def _window_pair(rng, sh, sw, c):
    img = rng.integers(0, 256, (sh, sw, c) if c > 1 else (sh, sw), dtype=np.uint8)
    return img, rng.random((sh, sw)).astype(np.float32)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("flip", [False, True])
def test_unit_window_equals_prepare_pair_bit_for_bit(c, flip):
    ch, cw = CROP
    img, dm = _window_pair(np.random.default_rng(c), ch, cw, c)
    xi, xg = prepare_pair_scaled(img, dm, ch, cw, D, flip)
    ri, rg = prepare_pair(img, dm, D, flip)
    assert xi.dtype == ri.dtype == np.float32 and xg.dtype == rg.dtype == np.float32
    assert xi.tobytes() == ri.tobytes() and xg.tobytes() == rg.tobytes()


def _dense_bilinear(n_in, n_out):
    """[n_out, n_in] float64 matrix of the cv2 INTER_LINEAR rule, from its definition: output o samples the source at
    (o + 0.5) * n_in / n_out - 0.5, a coordinate left of pixel 0 is pixel 0, right of the last pixel the last one."""
    m = np.zeros((n_out, n_in), dtype=np.float64)
    for o in range(n_out):
        src = (o + 0.5) * n_in / n_out - 0.5
        if src <= 0:
            m[o, 0] = 1.0
        elif src >= n_in - 1:
            m[o, n_in - 1] = 1.0
        else:
            lo = int(math.floor(src))
            m[o, lo] += 1.0 - (src - lo)
            m[o, lo + 1] += src - lo
    return m


# (sh, sw): magnified, shrunk, anisotropic, a one-pixel-wide window
@pytest.mark.parametrize("sh,sw", [(16, 24), (19, 29), (61, 95), (128, 192), (40, 30), (9, 150), (8, 1)])
@pytest.mark.parametrize("flip", [False, True])
def test_scaled_window_matches_a_dense_float64_reference(sh, sw, flip):
    ch, cw = CROP
    img, dm = _window_pair(np.random.default_rng(sh * 1000 + sw), sh, sw, 3)
    xi, xg = prepare_pair_scaled(img, dm, ch, cw, D, flip)
    assert xi.shape == (3, ch, cw) and xg.shape == (1, ch // D, cw // D)
    src = img.astype(np.float64) / 255.0
    dsrc = dm.astype(np.float64)
    if flip:
        src, dsrc = src[:, ::-1], dsrc[:, ::-1]
    ay, ax = _dense_bilinear(sh, ch), _dense_bilinear(sw, cw)
    ref = np.einsum("oy,yxc,px->cop", ay, src, ax)
    ref = (ref - IMAGENET_MEAN.astype(np.float64)[:, None, None]) / IMAGENET_STD.astype(np.float64)[:, None, None]
    # fp32 results of O(1) values (|x| <= 2.7): a few fp32 roundings, 2^-24 relative each
    assert np.abs(xi - ref).max() < 2e-6
    gy, gx = _dense_bilinear(sh, ch // D), _dense_bilinear(sw, cw // D)
    gref = gy @ dsrc @ gx.T * (sh * sw / ((ch // D) * (cw // D)))
    assert np.abs(xg[0] - gref).max() <= 4e-7 * np.abs(gref).max()


def test_result_depends_on_the_window_bytes_alone():
    """Taps clamp inside the window: the same window cut from two different surroundings gives the same sample."""
    rng = np.random.default_rng(2)
    big, dbig = _window_pair(rng, 90, 120, 3)
    other, dother = _window_pair(rng, 90, 120, 3)
    y0, x0, sh, sw = 13, 22, 50, 41
    other[y0:y0 + sh, x0:x0 + sw], dother[y0:y0 + sh, x0:x0 + sw] = big[y0:y0 + sh, x0:x0 + sw], dbig[y0:y0 + sh, x0:x0 + sw]
    a = prepare_pair_scaled(big[y0:y0 + sh, x0:x0 + sw], dbig[y0:y0 + sh, x0:x0 + sw], *CROP, D, True)
    b = prepare_pair_scaled(other[y0:y0 + sh, x0:x0 + sw], dother[y0:y0 + sh, x0:x0 + sw], *CROP, D, True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    with pytest.raises(ValueError):
        prepare_pair_scaled(big[:40, :40], dbig[:40, :41], *CROP, D, False)
    with pytest.raises(ValueError):
        prepare_pair_scaled(big[:40, :40], dbig[:40, :40], 30, 48, D, False)


# ---------------------------------------------------------------- density_to_gt_scaled
@pytest.mark.parametrize("sh,sw", [(32, 48), (16, 24), (19, 29), (61, 95), (128, 192), (9, 150), (4, 6)])
@pytest.mark.parametrize("flip", [False, True])
def test_density_to_gt_scaled_is_the_density_half(sh, sw, flip):
    ch, cw = CROP
    img, dm = _window_pair(np.random.default_rng(sh + sw), sh, sw, 3)
    g = density_to_gt_scaled(dm, ch, cw, D, flip)
    assert g.dtype == np.float32 and g.tobytes() == prepare_pair_scaled(img, dm, ch, cw, D, flip)[1].tobytes()
    if (sh, sw) == (ch, cw):
        assert g.tobytes() == density_to_gt(dm, ch, cw, D, flip).tobytes()
    const = np.full((sh, sw), 0.25, dtype=np.float32)
    want = np.float32(0.25 * sh * sw / ((ch // D) * (cw // D)))
    assert (density_to_gt_scaled(const, ch, cw, D, flip) == want).all()


def test_density_to_gt_scaled_reads_only_the_tap_rows():
    class Rows:                                                # a map that records the rows it is asked for
        def __init__(self, a):
            self.a, self.shape, self.ndim, self.seen = a, a.shape, a.ndim, []

        def __getitem__(self, idx):
            self.seen.append(np.asarray(idx))
            return self.a[idx]

    dm = np.random.default_rng(0).random((128, 192)).astype(np.float32)
    rec = Rows(dm)
    g = density_to_gt_scaled(rec, *CROP, D, False)
    assert g.tobytes() == density_to_gt_scaled(dm, *CROP, D, False).tobytes()
    assert len(rec.seen) == 1 and rec.seen[0].size == 2 * CROP[0] // D          # two tap rows per output row


# ---------------------------------------------------------------- the dataset
def _write(root, shapes, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    img_dir, gt_dir = os.path.join(root, "images"), os.path.join(root, "ground_truth")
    os.makedirs(img_dir), os.makedirs(gt_dir)
    imgs, dms = [], []
    for i, (h, w) in enumerate(shapes):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        dm = rng.random((h, w)).astype(np.float32)
        Image.fromarray(img).save(os.path.join(img_dir, f"IMG_{i}.png"))
        np.save(os.path.join(gt_dir, f"IMG_{i}.npy"), dm)
        imgs.append(img), dms.append(dm)
    return img_dir, gt_dir, imgs, dms


@pytest.fixture(scope="module")
def scale_set(tmp_path_factory):
    return _write(str(tmp_path_factory.mktemp("scale_set")), [(20, 30), (37, 53), (64, 80), (90, 120)])


@pytest.mark.parametrize("i", range(4))
def test_dataset_items_are_prepare_pair_scaled_of_the_drawn_windows(scale_set, i):
    img_dir, gt_dir, imgs, dms = scale_set
    K, (ch, cw) = 3, CROP
    kw = dict(seed=SEED, crop=CROP, crops_per_image=K, crop_scale=SCALE)
    x, gt = CrowdDataset(img_dir, gt_dir, D, "train", **kw)[(i, 2)]
    img, gts, wins = CrowdDataset(img_dir, gt_dir, D, "train", raw=True, **kw)[(i, 2)]
    assert tuple(x.shape) == (K, 3, ch, cw) and tuple(gt.shape) == (K, 1, ch // D, cw // D)
    assert torch.equal(img, torch.from_numpy(imgs[i])) and wins.dtype == torch.int64 and tuple(wins.shape) == (K, 5)
    assert torch.equal(gts, gt)                                # raw and CPU items describe the same samples
    h0, w0 = imgs[i].shape[:2]
    for k in range(K):
        sh, sw = scaled_window(h0, w0, ch, cw, scale_draw(SEED, 2, i, k, *SCALE))
        y0, x0, fl = crop_draw(SEED, 2, i, k, h0 - sh + 1, w0 - sw + 1)
        assert wins[k].tolist() == [y0, x0, int(fl), sh, sw]
        ri, rg = prepare_pair_scaled(imgs[i][y0:y0 + sh, x0:x0 + sw], dms[i][y0:y0 + sh, x0:x0 + sw], ch, cw, D, fl)
        assert x[k].numpy().tobytes() == ri.tobytes() and gt[k].numpy().tobytes() == rg.tobytes()
    assert len({tuple(w) for w in wins[:, 3:].tolist()}) > 1 or i == 0          # the K crops differ in scale


def test_draw_of_crop_k_does_not_depend_on_crops_per_image(scale_set):
    img_dir, gt_dir, _, _ = scale_set
    one = CrowdDataset(img_dir, gt_dir, D, "train", seed=SEED, raw=True, crop=CROP, crops_per_image=1,
                       crop_scale=SCALE)[3]
    four = CrowdDataset(img_dir, gt_dir, D, "train", seed=SEED, raw=True, crop=CROP, crops_per_image=4,
                        crop_scale=SCALE)[3]
    assert torch.equal(one[2][0], four[2][0]) and torch.equal(one[1][0], four[1][0])


def test_without_crop_scale_items_are_the_unscaled_ones(scale_set):
    img_dir, gt_dir, imgs, dms = scale_set
    from can_distributed_pytorch_amd.data.dataset import crop_window
    for raw in (False, True):
        off = CrowdDataset(img_dir, gt_dir, D, "train", seed=SEED, raw=raw, crop=CROP, crops_per_image=2,
                           crop_scale=None)
        plain = CrowdDataset(img_dir, gt_dir, D, "train", seed=SEED, raw=raw, crop=CROP, crops_per_image=2)
        for i in range(4):
            assert all(torch.equal(a, b) for a, b in zip(off[(i, 1)], plain[(i, 1)]))
    # ... and they are the unscaled rule: the window of crop_window at crop_draw's offset, zero-padded
    x, gt = CrowdDataset(img_dir, gt_dir, D, "train", seed=SEED, crop=CROP, crop_scale=None)[(1, 1)]
    vh, vw = crop_window(37, 53, *CROP)
    y0, x0, fl = crop_draw(SEED, 1, 1, 0, 37 - vh + 1, 53 - vw + 1)
    ri, rg = prepare_pair(imgs[1][y0:y0 + vh, x0:x0 + vw], dms[1][y0:y0 + vh, x0:x0 + vw], D, fl)
    assert x[0].numpy().tobytes() == ri.tobytes() and gt[0].numpy().tobytes() == rg.tobytes()
    # the test phase ignores both options; crop_scale without crop, and a bad range, are refused
    assert len(CrowdDataset(img_dir, gt_dir, D, "test", raw=True, crop=CROP, crop_scale=SCALE)[0]) == 3
    for bad in (dict(crop_scale=SCALE), dict(crop=CROP, crop_scale=(0.0, 1.0)), dict(crop=CROP, crop_scale=(2.0, 1.0)),
                dict(crop=CROP, crop_scale=(0.2, 1.0)), dict(crop=CROP, crop_scale=(1.0, 4.5))):
        with pytest.raises(ValueError):
            CrowdDataset(img_dir, gt_dir, D, "train", **bad)


def test_density_of_another_shape_is_refused(tmp_path):
    img_dir, gt_dir, _, _ = _write(str(tmp_path), [(64, 80)])
    np.save(os.path.join(gt_dir, "IMG_0.npy"), np.zeros((32, 40), np.float32))
    for raw in (False, True):
        with pytest.raises(ValueError, match="differs from its image"):
            CrowdDataset(img_dir, gt_dir, D, "train", seed=0, raw=raw, crop=CROP, crop_scale=SCALE)[0]


def _via_loader(ds, epoch, workers):
    from torch.utils.data import BatchSampler, DataLoader, SequentialSampler

    class S(SequentialSampler):
        pass

    s = S(ds)
    s.epoch = epoch
    dl = DataLoader(ds, batch_sampler=BatchSampler(EpochTaggedSampler(s), 2, drop_last=False), num_workers=workers,
                    collate_fn=crop_collate)
    return [b for b in dl]


def test_resumed_epoch_and_two_workers_draw_the_same_samples(scale_set):
    img_dir, gt_dir, _, _ = scale_set
    kw = dict(seed=SEED, crop=CROP, crops_per_image=2, crop_scale=SCALE)
    ds = CrowdDataset(img_dir, gt_dir, D, "train", **kw)
    ds.set_epoch(3)
    ran = [ds[i] for i in range(4)]                            # an uninterrupted run that reached epoch 3
    fresh = CrowdDataset(img_dir, gt_dir, D, "train", **kw)    # a resumed one
    assert all(torch.equal(a, b) for i in range(4) for a, b in zip(ran[i], fresh[(i, 3)]))
    assert not torch.equal(fresh[(3, 3)][0], fresh[(3, 4)][0])
    w0 = _via_loader(fresh, 3, workers=0)
    w2 = _via_loader(fresh, 3, workers=2)
    assert len(w0) == len(w2) == 2
    for a, b in zip(w0, w2):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(w0[1][0][2:], ran[3][0])


# ---------------------------------------------------------------- the packed collate
def test_packed_collate_scaled_layout(scale_set):
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, _unpack
    img_dir, gt_dir, imgs, _ = scale_set
    K, (ch, cw) = 2, CROP
    ds = CrowdDataset(img_dir, gt_dir, D, "train", seed=SEED, raw=True, crop=CROP, crops_per_image=K, crop_scale=SCALE)
    items = [ds[i] for i in (3, 0, 2)]
    packed = PackedCollate(crop=CROP, crop_scale=True)(items)
    buf, meta = packed
    n, ho, wo, goff, doff, n_img, scaled = meta
    assert (n, ho, wo, n_img, scaled) == (3 * K, ch, cw, 3, 1) and len(meta) == 7
    assert _unpack(packed)[1:] == ((n, ho, wo, goff, doff), "crop_scaled")
    sizes = [imgs[i].size for i in (3, 0, 2)]
    assert goff == -(-sum(sizes) // 16) * 16 and doff == -(-(goff + 4 * n * (ch // D) * (cw // D)) // 16) * 16
    assert buf.numel() == doff + 64 * n
    desc = buf[doff:].view(torch.int64).view(n, 8)
    off = 0
    for j, (img, gts, wins) in enumerate(items):
        assert torch.equal(buf[off:off + img.numel()], img.reshape(-1))
        for k in range(K):
            y0, x0, fl, sh, sw = wins[k].tolist()
            row = desc[j * K + k].tolist()
            assert row == [off, img.shape[0], img.shape[1], 3, fl, y0, x0, (sh << 32) | sw] and row[7] != 1
        off += img.numel()
    gt = buf[goff:goff + 4 * n * (ch // D) * (cw // D)].view(torch.float32).view(n, 1, ch // D, cw // D)
    assert torch.equal(gt, torch.cat([it[1] for it in items]))
    # [K,3] windows to a scaled collate, [K,5] windows to an unscaled one, crop_scale without crop
    plain = CrowdDataset(img_dir, gt_dir, D, "train", seed=SEED, raw=True, crop=CROP, crops_per_image=K)
    with pytest.raises(ValueError):
        PackedCollate(crop=CROP, crop_scale=True)([plain[2]])
    with pytest.raises(ValueError):
        PackedCollate(crop=CROP)([ds[2]])
    with pytest.raises(ValueError):
        PackedCollate(crop_scale=True)
    with pytest.raises(ValueError):
        _unpack((buf, meta[:6] + (0,)))
    # an unscaled cropped pack is what it was: six meta fields, slot 7 == 1
    pb, pm = PackedCollate(crop=CROP)([plain[2]])
    assert len(pm) == 6 and _unpack((pb, pm))[2] == "crop"
    assert pb[pm[4]:].view(torch.int64).view(K, 8)[:, 7].tolist() == [1] * K


def _assemble(imgs, gt, rows):
    """The documented layout, built independently: images | 16-byte-aligned fp32 ground truth | 16-byte-aligned int64
    descriptors.  Returns (bytes, defined): the alignment gaps carry no defined bytes."""
    ib = np.concatenate([np.asarray(im).reshape(-1) for im in imgs])
    goff = (ib.size + 15) // 16 * 16
    gb = np.ascontiguousarray(gt, dtype="<f4").reshape(-1).view(np.uint8)
    doff = (goff + gb.size + 15) // 16 * 16
    db = np.array(rows, dtype="<i8").reshape(-1).view(np.uint8)
    buf, defined = np.zeros(doff + db.size, np.uint8), np.zeros(doff + db.size, bool)
    for off, part in ((0, ib), (goff, gb), (doff, db)):
        buf[off:off + part.size], defined[off:off + part.size] = part, True
    return buf, defined, goff, doff


def test_packed_collate_bytes_of_all_three_kinds(scale_set):
    """An uncropped, a cropped and a scaled pack, every defined byte against a buffer assembled here."""
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate
    img_dir, gt_dir, imgs, _ = scale_set
    K = 2
    kw = dict(seed=SEED, raw=True)
    # uncropped: two images that resize to the same 32 x 48 (the 37 x 53 one of the set and a 39 x 50 x 4 one)
    rng = np.random.default_rng(2)
    im_a, g_a, fl_a = CrowdDataset(img_dir, gt_dir, D, "train", **kw)[1]
    im_b, g_b = torch.from_numpy(rng.integers(0, 256, (39, 50, 4), dtype=np.uint8)), torch.from_numpy(
        rng.random((1, 4, 6)).astype(np.float32))
    buf, meta = PackedCollate()([(im_a, g_a, fl_a), (im_b, g_b, True)])
    want, defined, goff, doff = _assemble([im_a, im_b], torch.stack([g_a, g_b]).numpy(),
                                          [[0, 37, 53, 3, int(fl_a), 0, 0, 0], [37 * 53 * 3, 39, 50, 4, 1, 0, 0, 0]])
    assert meta == (2, 32, 48, goff, doff) and buf.numel() == want.size
    assert np.array_equal(buf.numpy()[defined], want[defined])
    for scaled in (False, True):
        ds = CrowdDataset(img_dir, gt_dir, D, "train", crop=CROP, crops_per_image=K,
                          crop_scale=SCALE if scaled else None, **kw)
        items = [ds[2], ds[0], ds[3]]
        buf, meta = PackedCollate(crop=CROP, crop_scale=scaled)(items)
        rows, off = [], 0
        for img, _, wins in items:
            for w in wins.tolist():
                rows.append([off, img.shape[0], img.shape[1], 3, w[2], w[0], w[1], (w[3] << 32) | w[4] if scaled else 1])
            off += img.numel()
        want, defined, goff, doff = _assemble([it[0] for it in items], torch.cat([it[1] for it in items]).numpy(), rows)
        assert meta == (3 * K, *CROP, goff, doff, 3) + ((1,) if scaled else ()) and buf.numel() == want.size
        assert np.array_equal(buf.numpy()[defined], want[defined])


# ---------------------------------------------------------------- train.py
def test_train_py_crop_scale_option():
    sys.path.insert(0, ROOT)
    try:
        import train
    finally:
        sys.path.remove(ROOT)
    p = train.build_parser()
    assert p.parse_args([]).crop_scale is None
    assert p.parse_args(["--crop-size", "64x96"]).crop_scale is None
    a = p.parse_args(["--crop-size", "384x512", "--crop-scale", "0.75,1.33"])
    assert a.crop_scale == (0.75, 1.33) and a.crop_size == (384, 512)
    assert p.parse_args(["--crop-size", "64x96", "--crop-scale", "1,1"]).crop_scale == (1.0, 1.0)
    for bad in (["--crop-scale", "0.75,1.33"], ["--crop-size", "64x96", "--crop-scale", "0.75"],
                ["--crop-size", "64x96", "--crop-scale", "0.75,1.33,2"], ["--crop-size", "64x96", "--crop-scale", "a,b"],
                ["--crop-size", "64x96", "--crop-scale", "0,1"], ["--crop-size", "64x96", "--crop-scale", "-1,1"],
                ["--crop-size", "64x96", "--crop-scale", "1.5,1"], ["--crop-size", "64x96", "--crop-scale", "0.2,1"],
                ["--crop-size", "64x96", "--crop-scale", "1,4.5"], ["--crop-size", "64x96", "--crop-scale", "nan,1"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
