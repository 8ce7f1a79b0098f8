"""Random-crop training data on the CPU: the stateless crop draws, CrowdDataset(crop=...) against prepare_pair on the
window's slices, the cropped PackedCollate layout, resumed / multi-worker draws and the train.py options."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from can_distributed_pytorch_amd.data import CrowdDataset
from can_distributed_pytorch_amd.data.dataset import (EpochTaggedSampler, crop_collate, crop_draw, crop_window,
                                                      density_to_gt)
from can_distributed_pytorch_amd.data.transforms import prepare_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP = (32, 48)
SEED = 11


def _pad(a, h, w):
    out = np.zeros(a.shape[:-2] + (h, w), dtype=a.dtype)
    out[..., :a.shape[-2], :a.shape[-1]] = a
    return out


def _write(root, shapes, gt_shapes=None, seed=0):
    """PNG images (lossless: the decoded bytes are the written ones) + density maps; returns the arrays."""
    rng = np.random.default_rng(seed)
    img_dir, gt_dir = os.path.join(root, "img"), os.path.join(root, "gt")
    os.makedirs(img_dir)
    os.makedirs(gt_dir)
    imgs, dms = [], []
    for i, shp in enumerate(shapes):
        a = rng.integers(0, 256, shp, dtype=np.uint8)
        Image.fromarray(a).save(os.path.join(img_dir, f"IMG_{i}.png"))
        d = rng.random((gt_shapes or shapes)[i][:2]).astype(np.float32)
        np.save(os.path.join(gt_dir, f"IMG_{i}.npy"), d)
        imgs.append(a)
        dms.append(d)
    return img_dir, gt_dir, imgs, dms


# ---------------------------------------------------------------- draws
def test_draws_are_a_pure_function_of_seed_epoch_index_k():
    a = [crop_draw(3, 2, 7, k, 9, 9) for k in range(4)]
    assert a == [crop_draw(3, 2, 7, k, 9, 9) for k in range(4)]
    others = [[crop_draw(s, e, i, k, 1000, 1000) for k in range(4)]
              for s, e, i in ((3, 2, 7), (4, 2, 7), (3, 3, 7), (3, 2, 8))]
    assert all(others[0] != o for o in others[1:])
    assert len({d[:2] for d in others[0]}) == 4                # the K crops of one image differ


def test_draw_of_crop_k_does_not_depend_on_crops_per_image(tmp_path):
    img_dir, gt_dir, _, _ = _write(str(tmp_path), [(77, 101, 3)])
    one = CrowdDataset(img_dir, gt_dir, 8, "train", seed=SEED, crop=CROP, crops_per_image=1)[0]
    four = CrowdDataset(img_dir, gt_dir, 8, "train", seed=SEED, crop=CROP, crops_per_image=4)[0]
    assert tuple(four[0].shape) == (4, 3, 32, 48) and tuple(four[1].shape) == (4, 1, 4, 6)
    assert torch.equal(one[0][0], four[0][0]) and torch.equal(one[1][0], four[1][0])


def test_draw_range_and_uniformity():
    h0, w0 = 40, 56
    vh, vw = crop_window(h0, w0, *CROP)
    assert (vh, vw) == CROP
    ny, nx = h0 - vh + 1, w0 - vw + 1
    assert ny == 9 and nx == 9
    draws = [crop_draw(SEED, 0, i, 0, ny, nx) for i in range(2000)]
    ys, xs = np.array([d[0] for d in draws]), np.array([d[1] for d in draws])
    assert ys.min() == 0 and ys.max() == h0 - vh and xs.min() == 0 and xs.max() == w0 - vw
    rate = np.mean([d[2] for d in draws])
    assert abs(rate - 0.5) <= 0.05, rate
    for v in (ys, xs):
        assert np.bincount(v, minlength=9).min() >= 0.5 * 2000 / 9, np.bincount(v, minlength=9)
    # an image smaller than the crop has one position per short axis
    assert crop_window(24, 70, *CROP) == (24, 48) and crop_window(20, 30, *CROP) == (16, 24)
    assert all(crop_draw(SEED, 0, i, 0, 1, 1)[:2] == (0, 0) for i in range(50))


# ---------------------------------------------------------------- dataset
SHAPES = [(77, 101, 3), (50, 70), (24, 70, 3), (20, 30, 3)]


@pytest.fixture(scope="module")
def crop_set(tmp_path_factory):
    return _write(str(tmp_path_factory.mktemp("crop_set")), SHAPES)


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_dataset_crops_equal_prepare_pair_on_the_slices(crop_set, i):
    img_dir, gt_dir, imgs, dms = crop_set
    K, (ch, cw) = 3, CROP
    ds = CrowdDataset(img_dir, gt_dir, 8, "train", seed=SEED, crop=CROP, crops_per_image=K)
    ds.set_epoch(2)
    x, gt = ds[i]
    assert tuple(x.shape) == (K, 3, ch, cw) and tuple(gt.shape) == (K, 1, ch // 8, cw // 8)
    assert x.dtype == torch.float32 and gt.dtype == torch.float32
    h0, w0 = imgs[i].shape[:2]
    vh, vw = crop_window(h0, w0, ch, cw)
    for k in range(K):
        y0, x0, fl = crop_draw(SEED, 2, i, k, h0 - vh + 1, w0 - vw + 1)
        assert 0 <= y0 <= h0 - vh and 0 <= x0 <= w0 - vw
        ri, rg = prepare_pair(imgs[i][y0:y0 + vh, x0:x0 + vw], dms[i][y0:y0 + vh, x0:x0 + vw], 8, fl)
        assert ri.shape == (3, vh, vw)
        assert np.array_equal(x[k].numpy(), _pad(ri, ch, cw))
        assert np.array_equal(gt[k].numpy(), _pad(rg, ch // 8, cw // 8))


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_raw_dataset_carries_the_image_once_and_the_same_ground_truth(crop_set, i):
    img_dir, gt_dir, imgs, _ = crop_set
    K = 3
    cpu = CrowdDataset(img_dir, gt_dir, 8, "train", seed=SEED, crop=CROP, crops_per_image=K)[i]
    img, gts, wins = CrowdDataset(img_dir, gt_dir, 8, "train", seed=SEED, raw=True, crop=CROP, crops_per_image=K)[i]
    assert img.dtype == torch.uint8 and np.array_equal(img.numpy(), imgs[i])
    assert tuple(gts.shape) == tuple(cpu[1].shape) and float((gts - cpu[1]).abs().max()) <= 1e-6
    h0, w0 = imgs[i].shape[:2]
    vh, vw = crop_window(h0, w0, *CROP)
    assert wins.dtype == torch.int64
    assert wins.tolist() == [[y0, x0, int(fl)] for y0, x0, fl in
                             (crop_draw(SEED, 0, i, k, h0 - vh + 1, w0 - vw + 1) for k in range(K))]


def test_density_of_another_shape_is_refused_in_crop_mode(tmp_path):
    img_dir, gt_dir, _, _ = _write(str(tmp_path), [(64, 80, 3)], gt_shapes=[(32, 40)])
    for raw in (False, True):
        with pytest.raises(ValueError):
            CrowdDataset(img_dir, gt_dir, 8, "train", seed=0, raw=raw, crop=CROP)[0]
        CrowdDataset(img_dir, gt_dir, 8, "train", seed=0, raw=raw)[0]          # uncropped: resized, as before


def test_test_phase_ignores_crop(crop_set):
    img_dir, gt_dir, imgs, dms = crop_set
    x, gt = CrowdDataset(img_dir, gt_dir, 8, "test", crop=CROP, crops_per_image=4)[0]
    ri, rg = prepare_pair(imgs[0], dms[0], 8, False)
    assert np.array_equal(x.numpy(), ri) and np.array_equal(gt.numpy(), rg)
    assert len(CrowdDataset(img_dir, gt_dir, 8, "test", raw=True, crop=CROP)[0]) == 3      # (img, gt, flip)
    with pytest.raises(ValueError):
        CrowdDataset(img_dir, gt_dir, 8, "train", crop=(20, 48))
    with pytest.raises(ValueError):
        CrowdDataset(img_dir, gt_dir, 8, "train", crop=CROP, crops_per_image=0)


def test_crop_collate_concatenates_the_stacks(crop_set):
    img_dir, gt_dir, _, _ = crop_set
    ds = CrowdDataset(img_dir, gt_dir, 8, "train", seed=SEED, crop=CROP, crops_per_image=3)
    a, b = ds[0], ds[3]
    x, gt = crop_collate([a, b])
    assert tuple(x.shape) == (6, 3, 32, 48) and tuple(gt.shape) == (6, 1, 4, 6)
    assert torch.equal(x[:3], a[0]) and torch.equal(x[3:], b[0]) and torch.equal(gt[3:], b[1])


# ---------------------------------------------------------------- packing
def test_packed_collate_crop_stores_each_image_once(crop_set):
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, _unpack
    img_dir, gt_dir, imgs, _ = crop_set
    K = 3
    ds = CrowdDataset(img_dir, gt_dir, 8, "train", seed=SEED, raw=True, crop=CROP, crops_per_image=K)
    items = [ds[0], ds[1]]                                    # 77x101x3 and gray 50x70
    packed = PackedCollate(crop=CROP)(items)
    buf, meta = packed
    n, ho, wo, goff, doff = meta[:5]
    assert (n, ho, wo) == (6, 32, 48) and len(meta) == 6 and meta[5] == 2
    assert buf.dtype == torch.uint8 and goff % 16 == 0 and doff % 16 == 0 and buf.numel() == doff + 64 * n
    assert _unpack(packed)[2] == "crop"
    nb0, nb1 = 77 * 101 * 3, 50 * 70
    assert goff == -(-(nb0 + nb1) // 16) * 16                 # both images once, nothing else ahead of the gt
    assert np.array_equal(buf[:nb0].numpy(), imgs[0].reshape(-1))
    assert np.array_equal(buf[nb0:nb0 + nb1].numpy(), imgs[1].reshape(-1))
    desc = buf[doff:].view(torch.int64).view(n, 8)
    assert desc[:, 0].tolist() == [0, 0, 0, nb0, nb0, nb0]    # K descriptors share one image offset
    assert desc[:3, 1:4].tolist() == [[77, 101, 3]] * 3 and desc[3:, 1:4].tolist() == [[50, 70, 1]] * 3
    assert desc[:, 7].tolist() == [1] * 6
    wins = torch.cat([items[0][2], items[1][2]])
    assert torch.equal(desc[:, 5:7], wins[:, :2]) and torch.equal(desc[:, 4], wins[:, 2])
    gt = buf[goff:goff + 4 * n * 4 * 6].view(torch.float32).view(n, 1, 4, 6)
    assert torch.equal(gt, torch.cat([items[0][1], items[1][1]]))


def test_packed_collate_without_crop_is_unchanged():
    """The uncropped pack, field by field, as the parent wrote it (the layout tests/test_data.py pins)."""
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, _unpack
    rng = np.random.default_rng(4)
    samples = []
    for i, shp in enumerate([(77, 101, 3), (79, 103)]):       # both -> 72 x 96
        img = rng.integers(0, 256, shp, dtype=np.uint8)
        dm = rng.random(shp[:2]).astype(np.float32)
        samples.append((torch.from_numpy(img), torch.from_numpy(density_to_gt(dm, shp[0], shp[1], 8, bool(i))), bool(i)))
    packed = PackedCollate()(samples)
    buf, meta = packed
    nb0, nb1 = 77 * 101 * 3, 79 * 103
    goff = -(-(nb0 + nb1) // 16) * 16
    doff = -(-(goff + 4 * 2 * 9 * 12) // 16) * 16
    assert meta == (2, 72, 96, goff, doff) and buf.numel() == doff + 128
    assert _unpack(packed)[2] == "batch"
    assert torch.equal(buf[:nb0 + nb1], torch.cat([s[0].reshape(-1) for s in samples]))
    assert torch.equal(buf[goff:goff + 4 * 216].view(torch.float32), torch.stack([s[1] for s in samples]).reshape(-1))
    assert buf[doff:].view(torch.int64).view(2, 8).tolist() == [[0, 77, 101, 3, 0, 0, 0, 0], [nb0, 79, 103, 1, 1, 0, 0, 0]]


# ---------------------------------------------------------------- resume / workers
def _crops_via_loader(ds, epoch, workers):
    from torch.utils.data import BatchSampler, DataLoader, DistributedSampler
    smp = DistributedSampler(ds, num_replicas=1, rank=0, shuffle=True, seed=0)
    smp.set_epoch(epoch)
    dl = DataLoader(ds, batch_sampler=BatchSampler(EpochTaggedSampler(smp), 1, drop_last=False), num_workers=workers,
                    collate_fn=crop_collate)
    return {i: x for i, (x, _) in zip(list(smp), dl)}


def test_resumed_epoch_and_two_workers_draw_the_same_crops(tmp_path):
    img_dir, gt_dir, imgs, dms = _write(str(tmp_path), [(77, 101, 3)] * 6, seed=2)
    ds = CrowdDataset(img_dir, gt_dir, 8, "train", seed=SEED, crop=CROP, crops_per_image=2)
    ds.set_epoch(3)
    fresh = CrowdDataset(img_dir, gt_dir, 8, "train", seed=SEED, crop=CROP, crops_per_image=2)     # a resumed run
    fresh.set_epoch(3)
    e0 = CrowdDataset(img_dir, gt_dir, 8, "train", seed=SEED, crop=CROP, crops_per_image=2)[0][0]
    assert torch.equal(ds[0][0], fresh[0][0]) and not torch.equal(ds[0][0], e0)
    y0, x0, fl = crop_draw(SEED, 3, 0, 1, 77 - 32 + 1, 101 - 48 + 1)
    assert np.array_equal(fresh[0][0][1].numpy(), prepare_pair(imgs[0][y0:y0 + 32, x0:x0 + 48],
                                                               dms[0][y0:y0 + 32, x0:x0 + 48], 8, fl)[0])
    w0 = _crops_via_loader(fresh, 3, workers=0)
    w2 = _crops_via_loader(fresh, 3, workers=2)
    assert sorted(w0) == sorted(w2) == list(range(6))
    assert all(torch.equal(w0[i], w2[i]) for i in w0)         # the epoch travels with the index into the workers
    assert all(torch.equal(w0[i], ds[i][0]) for i in w0)
    # no worker replays another's draws: all 12 windows of the epoch are distinct
    draws = {crop_draw(SEED, 3, i, k, 46, 54)[:2] for i in range(6) for k in range(2)}
    assert len(draws) == 12


# ---------------------------------------------------------------- parser
def _parser():
    sys.path.insert(0, ROOT)
    try:
        import train
    finally:
        sys.path.remove(ROOT)
    return train.build_parser()


def test_parser_defaults_and_argument_errors(capsys):
    p = _parser()
    a = p.parse_args([])
    assert a.crop_size is None and a.crops_per_image == 1
    a = p.parse_args(["--crop-size", "384x512", "--crops-per-image", "4", "--batch-size", "8"])
    assert a.crop_size == (384, 512) and a.crops_per_image == 4
    for bad in (["--crop-size", "64x96", "--synthetic", "64x64"], ["--crop-size", "60x96"], ["--crop-size", "64x100"],
                ["--crop-size", "64x96", "--crops-per-image", "0"], ["--crop-size", "64"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    capsys.readouterr()
