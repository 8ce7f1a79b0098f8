"""ROI masks and GAME on the CPU: the loop references of tests/roi_reference.py checked against their own definitions,
data/transforms.py:roi_weights bit for bit against them, the torch path of engine/metrics.py:count_metrics,
CrowdDataset(roi=True) items of every kind, the roi pack's bytes, and train.py --impl torch with the new options."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import roi_reference as RR
from can_distributed_pytorch_amd.data import CrowdDataset
from can_distributed_pytorch_amd.data.dataset import crop_collate
from can_distributed_pytorch_amd.data.transforms import roi_weights, roi_weights_padded
from can_distributed_pytorch_amd.engine.metrics import count_metrics, count_metrics_torch, split_gt, weighted_sq_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _windows():
    """(mask h0, w0, y0, x0, sh, sw, rows, cols) of the window set the GPU test renders as well."""
    out = []
    for ch, cw, s in RR.SCALED_WINDOWS:
        sh, sw = RR.window_of(ch, cw, s)
        out.append((sh + 5, sw + 9, 3, 7, sh, sw, ch // 8, cw // 8))
    h0, w0 = RR.WHOLE_IMAGE
    out.append((h0, w0, 0, 0, h0, w0, h0 // 8, w0 // 8))
    return out


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("sh,rows", [(1, 1), (3, 2), (7, 3), (16, 2), (37, 4), (64, 17), (5, 8), (544, 17)])
def test_overlap_numerators_sum_to_the_extent(sh, rows):
    for i in range(rows):
        assert sum(RR.overlap(i, t, sh, rows) for t in range(sh)) == sh
    for t in range(sh):
        assert sum(RR.overlap(i, t, sh, rows) for i in range(rows)) == rows


@pytest.mark.parametrize("win", _windows(), ids=lambda w: "x".join(str(v) for v in w))
def test_reference_properties(win):
    h0, w0, y0, x0, sh, sw, rows, cols = win
    ones = RR.roi_weights_ref(RR.make_mask(h0, w0, 1, "ones"), y0, x0, sh, sw, rows, cols, False)
    assert np.array_equal(_bits(ones), _bits(np.ones((rows, cols))))                # an all-255 mask: exactly 1.0
    for kind in ("binary", "frac"):
        mask = RR.make_mask(h0, w0, 2, kind)
        m = RR.roi_weights_ref(mask, y0, x0, sh, sw, rows, cols, False)
        mean = mask[y0:y0 + sh, x0:x0 + sw].astype(np.float64).mean()
        # every cell is one rounding of a value in [0, 1]: the mean of the cells is the window's to rows * cols / 2 ulp
        assert abs(m.astype(np.float64).mean() * 255 - mean) <= 255 * 2.0 ** -24
        assert m.min() >= 0 and m.max() <= 1
        flipped = RR.roi_weights_ref(mask, y0, x0, sh, sw, rows, cols, True)
        assert np.array_equal(_bits(flipped), _bits(m[:, ::-1]))


def test_reference_padding_cells_are_zero():
    (h0, w0), (ch, cw) = RR.SMALL_IMAGE, RR.SMALL_CROP
    mask = RR.make_mask(h0, w0, 3, "ones")
    for flip in (False, True):
        m = RR.roi_weights_padded_ref(mask, 2, 1, ch, cw, 8, flip)
        vh, vw = min(ch, h0 // 8 * 8), min(cw, w0 // 8 * 8)
        assert m.shape == (ch // 8, cw // 8) and (vh, vw) == (16, 40)
        assert np.all(m[:vh // 8, :vw // 8] == 1) and np.all(m[vh // 8:] == 0) and np.all(m[:, vw // 8:] == 0)


# ------------------------------------------------------------------------------------------ transforms.roi_weights
@pytest.mark.parametrize("kind", ["binary", "frac"])
@pytest.mark.parametrize("win", _windows(), ids=lambda w: "x".join(str(v) for v in w))
def test_roi_weights_equals_the_reference_bit_for_bit(win, kind):
    h0, w0, y0, x0, sh, sw, rows, cols = win
    mask = RR.make_mask(h0, w0, 5, kind)
    for flip in (False, True):
        got = roi_weights(mask, y0, x0, sh, sw, rows, cols, flip)
        assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(_bits(got), _bits(RR.roi_weights_ref(mask, y0, x0, sh, sw, rows, cols, flip)))


@pytest.mark.parametrize("kind", ["binary", "frac"])
def test_roi_weights_padded_equals_the_reference(kind):
    (h0, w0), (ch, cw) = RR.SMALL_IMAGE, RR.SMALL_CROP
    mask = RR.make_mask(h0, w0, 6, kind)
    for flip in (False, True):
        got = roi_weights_padded(mask, 4, 3, ch, cw, 8, flip)
        assert np.array_equal(_bits(got), _bits(RR.roi_weights_padded_ref(mask, 4, 3, ch, cw, 8, flip)))


def test_roi_weights_refuses_bad_arguments():
    mask = RR.make_mask(20, 30, 0, "binary")
    with pytest.raises(ValueError):
        roi_weights(mask, 0, 0, 21, 30, 2, 3)
    with pytest.raises(ValueError):
        roi_weights(mask, 0, 0, 0, 30, 2, 3)
    with pytest.raises(ValueError):
        roi_weights(mask.astype(np.float32), 0, 0, 20, 30, 2, 3)


# ---------------------------------------------------------------------------------------------------------- metrics
@pytest.mark.parametrize("n,h,w", RR.METRIC_SHAPES)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_count_metrics_torch_path(n, h, w, masked):
    et, gt, m = RR.metric_inputs(n, h, w, seed=h * w + n, exact=True)
    ref, _ = RR.count_metrics_ref(et, gt, m if masked else None)
    gt_t = torch.stack([gt, m], 1) if masked else gt[:, None]
    got = count_metrics(et[:, None], gt_t)
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, 6)
    assert torch.equal(got, ref)                                  # exactly representable sums: any order agrees
    assert torch.equal(got, count_metrics_torch(et[:, None], gt_t))
    assert torch.equal(got[:, 2], (got[:, 0] - got[:, 1]).abs())  # GAME_0 = |E - G|
    assert bool((got[:, 2:-1] <= got[:, 3:]).all())               # GAME_0 <= GAME_1 <= GAME_2 <= GAME_3
    et, gt, m = RR.metric_inputs(n, h, w, seed=7 + h, exact=False)
    ref, bound = RR.count_metrics_ref(et, gt, m if masked else None)
    got = count_metrics(et[:, None], torch.stack([gt, m], 1) if masked else gt[:, None])
    assert bool(((got - ref).abs() <= bound).all())
    assert bool((got[:, 2:-1] <= got[:, 3:] + bound[:, 3:]).all())


def test_split_gt_and_weighted_loss():
    g = torch.Generator().manual_seed(0)
    et, gt, m = (torch.rand(2, 1, 5, 7, generator=g) for _ in range(3))
    a, b = split_gt(gt)
    assert a is gt and b is None
    a, b = split_gt(torch.cat([gt, m], 1))
    assert torch.equal(a, gt) and torch.equal(b, m)
    with pytest.raises(ValueError):
        split_gt(torch.zeros(2, 3, 5, 7))
    assert torch.equal(weighted_sq_loss(et, gt), torch.nn.MSELoss(reduction="sum")(et, gt))
    assert torch.equal(weighted_sq_loss(et, torch.cat([gt, m], 1)), ((et - gt) ** 2 * m).sum())
    one = weighted_sq_loss(et, torch.cat([gt, torch.ones_like(m)], 1))
    assert torch.allclose(one, weighted_sq_loss(et, gt), rtol=1e-6)


# ------------------------------------------------------------------------------------------------ dataset / collate
SIZES = [(40, 56), (21, 45), (37, 53)]
CROP = (32, 40)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return RR.write_folder(str(tmp_path_factory.mktemp("roi")), SIZES, seed=3)


KINDS = [dict(), dict(crop=CROP, crops_per_image=2), dict(crop=CROP, crops_per_image=2, crop_scale=(0.5, 2.0)),
         dict(crop=CROP, crops_per_image=2, gt_from_heads=True),
         dict(crop=CROP, crops_per_image=2, crop_scale=(0.5, 2.0), gt_from_heads=True),
         dict(crop=CROP, crops_per_image=2, photo_jitter=(0.2, 0.3, 1.5), gray_prob=0.5)]
KIND_IDS = ["whole", "crop", "scaled", "crop+heads", "scaled+heads", "crop+photo"]


@pytest.mark.parametrize("kw", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("phase", ["train", "test"])
def test_dataset_items_of_every_kind(folder, kw, phase):
    """raw=False: the gt gains the weight plane as channel 1, channel 0 and the image are the plain dataset's; raw=True:
    the image becomes [H0, W0, 4] with the mask as alpha, nothing else in the item changes."""
    from can_distributed_pytorch_amd.data.density import roi_path
    img_root, gt_root = folder
    plain = CrowdDataset(img_root, gt_root, 8, phase=phase, seed=5, **kw)
    roi = CrowdDataset(img_root, gt_root, 8, phase=phase, seed=5, roi=True, **kw)
    raw_plain = CrowdDataset(img_root, gt_root, 8, phase=phase, seed=5, raw=True, **kw)
    raw_roi = CrowdDataset(img_root, gt_root, 8, phase=phase, seed=5, raw=True, roi=True, **kw)
    cropped = "crop" in kw and phase == "train"
    for i, (h0, w0) in enumerate(SIZES):
        mask = np.load(roi_path(os.path.join(gt_root, f"IMG_{i + 1}.npy")))
        (im, gt), (im2, gt2) = plain[i], roi[i]
        assert torch.equal(im, im2)
        if cropped:
            assert tuple(gt2.shape) == (2, 2, CROP[0] // 8, CROP[1] // 8)
            assert torch.equal(gt2[:, 0:1], gt)
        else:
            assert tuple(gt2.shape) == (2, h0 // 8, w0 // 8)
            assert torch.equal(gt2[0:1], gt)
        w = gt2[:, 1] if cropped else gt2[1]
        assert w.dtype == torch.float32 and float(w.min()) >= 0 and float(w.max()) <= 1
        a, b = raw_plain[i], raw_roi[i]
        assert len(a) == len(b) and tuple(b[0].shape) == (h0, w0, 4) and b[0].dtype == torch.uint8
        assert torch.equal(b[0][:, :, :3], a[0]) and np.array_equal(b[0][:, :, 3].numpy(), mask)
        for u, v in zip(a[1:], b[1:]):
            assert torch.equal(torch.as_tensor(u), torch.as_tensor(v))
        if cropped:
            # the weights of the raw item's windows, by the reference
            for k, row in enumerate(b[2].tolist()):
                y0, x0, fl = row[:3]
                want = RR.roi_weights_ref(mask, y0, x0, row[3], row[4], CROP[0] // 8, CROP[1] // 8, bool(fl)) \
                    if len(row) == 5 else RR.roi_weights_padded_ref(mask, y0, x0, *CROP, 8, bool(fl))
                assert np.array_equal(_bits(w[k].numpy()), _bits(want))
        else:
            want = RR.roi_weights_ref(mask, 0, 0, h0, w0, h0 // 8, w0 // 8, bool(a[2]))
            assert np.array_equal(_bits(w.numpy()), _bits(want))


def test_gray_and_rgba_images_are_expanded(tmp_path):
    from PIL import Image
    from can_distributed_pytorch_amd.data.density import roi_path
    img_root, gt_root = str(tmp_path / "images"), str(tmp_path / "ground_truth")
    os.makedirs(img_root)
    os.makedirs(gt_root)
    g = np.random.default_rng(0)
    gray = g.integers(0, 256, (24, 32), dtype=np.uint8)
    rgba = g.integers(0, 256, (24, 32, 4), dtype=np.uint8)
    Image.fromarray(gray).save(os.path.join(img_root, "A.png"))
    Image.fromarray(rgba).save(os.path.join(img_root, "B.png"))
    mask = RR.make_mask(24, 32, 1, "frac")
    for name in "AB":
        np.save(os.path.join(gt_root, name + ".npy"), np.zeros((24, 32), dtype=np.float32))
        np.save(roi_path(os.path.join(gt_root, name + ".npy")), mask)
    ds = CrowdDataset(img_root, gt_root, 8, phase="test", raw=True, roi=True)
    a, b = ds[0][0].numpy(), ds[1][0].numpy()
    assert a.shape == b.shape == (24, 32, 4)
    assert all(np.array_equal(a[:, :, c], gray) for c in range(3)) and np.array_equal(a[:, :, 3], mask)
    assert np.array_equal(b[:, :, :3], rgba[:, :, :3]) and np.array_equal(b[:, :, 3], mask)     # own alpha replaced


def test_roi_pack_is_the_rgba_pack_of_the_same_bytes(folder):
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate
    img_root, gt_root = folder
    for kw, ckw in [(dict(), dict()), (dict(crop=CROP, crops_per_image=2), dict(crop=CROP)),
                    (dict(crop=CROP, crops_per_image=2, crop_scale=(0.5, 2.0), gt_from_heads=True),
                     dict(crop=CROP, crop_scale=True, gt_from_heads=True))]:
        ds = CrowdDataset(img_root, gt_root, 8, phase="train", seed=5, raw=True, roi=True, **kw)
        items = [ds[i] for i in ((0,) if not kw else (0, 1, 2))]
        rgba = [(torch.from_numpy(np.array(it[0].numpy())),) + tuple(it[1:]) for it in items]   # plain RGBA arrays
        collate = PackedCollate(**ckw)
        (buf, meta), (buf2, meta2) = collate(items), collate(rgba)
        assert meta == meta2 and buf.numel() == buf2.numel()
        n, ho, wo, goff, doff = meta[:5]
        ioff = sum(it[0].numel() for it in items)
        # (the alignment gaps behind the images and the ground truth are not written by the collate)
        for lo, hi in ((0, ioff), (goff, goff + 4 * n * (ho // 8) * (wo // 8)), (doff, buf.numel())):
            assert torch.equal(buf[lo:hi], buf2[lo:hi])
        assert ioff == sum(4 * h * w for h, w in SIZES[:len(items)])
        desc = buf[meta[4]:meta[4] + 64 * n].view(torch.int64).view(n, 8)
        assert bool((desc[:, 3] == 4).all())


def test_missing_or_misshaped_mask_is_a_value_error(tmp_path):
    from can_distributed_pytorch_amd.data.density import roi_path
    img_root, gt_root = RR.write_folder(str(tmp_path), [(24, 32), (24, 32)], masks=False)
    for raw in (False, True):
        ds = CrowdDataset(img_root, gt_root, 8, phase="train", raw=raw, roi=True)
        with pytest.raises(ValueError, match=r"IMG_1\.roi\.npy"):
            ds[0]
    np.save(roi_path(os.path.join(gt_root, "IMG_1.npy")), np.zeros((24, 31), dtype=np.uint8))
    np.save(roi_path(os.path.join(gt_root, "IMG_2.npy")), np.zeros((24, 32), dtype=np.float32))
    ds = CrowdDataset(img_root, gt_root, 8, phase="train", crop=(16, 24), roi=True)
    for i in (0, 1):
        with pytest.raises(ValueError, match=rf"IMG_{i + 1}\.roi\.npy"):
            ds[i]
    assert len(CrowdDataset(img_root, gt_root, 8, phase="train")[0]) == 2                      # off: no mask is opened


def test_crop_collate_keeps_both_channels(folder):
    img_root, gt_root = folder
    ds = CrowdDataset(img_root, gt_root, 8, phase="train", seed=5, crop=CROP, crops_per_image=2, roi=True)
    img, gt = crop_collate([ds[0], ds[1]])
    assert tuple(img.shape) == (4, 3, *CROP) and tuple(gt.shape) == (4, 2, CROP[0] // 8, CROP[1] // 8)


# --------------------------------------------------------------------------------------------------------- train.py
def _parser():
    sys.path.insert(0, ROOT)
    import train
    return train.build_parser()


def test_parser_errors(capsys):
    p = _parser()
    ns = p.parse_args([])
    assert ns.roi_masks is False and ns.eval_game is None
    assert p.parse_args(["--roi-masks", "--eval-game", "3"]).eval_game == 3
    assert p.parse_args(["--eval-game", "0"]).eval_game == 0
    for bad in (["--roi-masks", "--synthetic", "64x64"], ["--eval-game", "4"], ["--eval-game", "-1"],
                ["--eval-game", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    assert "--roi-masks" in capsys.readouterr().err


def test_train_py_torch_roi_masks_and_game(tmp_path):
    """Two steps of --impl torch on a small JPEG folder with masks: the epoch record carries mae, rmse, game1..game3,
    GAME is monotone and the best checkpoint is written."""
    data = tmp_path / "data"
    RR.write_folder(str(data / "train_data"), [(40, 56), (21, 45)], seed=1, heads=False)
    RR.write_folder(str(data / "test_data"), [(37, 53), (40, 56)], seed=2, heads=False)
    ck = tmp_path / "ck"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--data_root", str(data), "--epochs", "1", "--batch-size", "1",
           "--impl", "torch", "--device", "cpu", "--num-workers", "0", "--wandb", "false", "--show", "false",
           "--roi-masks", "--eval-game", "3", "--crop-size", "16x24", "--init_checkpoint", "",
           "--checkpoint-dir", str(ck), "--log-jsonl", str(ck / "metrics.jsonl")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    ep = [x for x in (json.loads(x) for x in open(ck / "metrics.jsonl")) if x["kind"] == "epoch"]
    assert len(ep) == 1
    rec = ep[0]
    vals = [rec[k] for k in ("loss", "mae", "rmse", "game1", "game2", "game3")]
    assert all(np.isfinite(v) for v in vals) and rec["roi_masks"] is True
    assert rec["mae"] <= rec["game1"] <= rec["game2"] <= rec["game3"] and rec["rmse"] >= rec["mae"] - 1e-9
    assert os.path.exists(ck / "epoch_0.pth")
