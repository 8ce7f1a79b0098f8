"""Random-crop input pipeline on the GPU: the crop kernel against the CPU transform on the window's slices, the
cropped pack through preprocess_packed / AheadPrep, the untouched resize path, refused arguments, and train.py
end to end on a generated mixed-size JPEG set."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH, CW, D = 32, 48, 8
# (H0, W0, C): gray, RGB, RGBA, shorter than the crop (padded rows), smaller in both axes (padded rows and columns)
SOURCES = [(37, 53, 1), (64, 80, 3), (40, 56, 4), (24, 70, 3), (20, 30, 3)]


def _window(h0, w0):
    return min(CH, h0 // D * D), min(CW, w0 // D * D)


def _hand_pack(order=SOURCES, seed=3):
    """A cropped pack built by hand, K = 3 per image: windows at (0, 0), at the far corner (H0-vh, W0-vw) and one in
    between, flips mixed.  The LAST descriptor is the far corner of the last image of the buffer, unflipped and
    flipped: a read past the window there lands in the ground truth / descriptor bytes.  Returns (packed, refs)
    with refs[n] = (prepare_pair image, ground truth) of output sample n, zero-padded."""
    from can_distributed_pytorch_amd.data.dataset import density_to_gt
    from can_distributed_pytorch_amd.data.transforms import prepare_pair
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate
    rng = np.random.default_rng(seed)
    items, refs = [], []
    for j, (h0, w0, c) in enumerate(order):
        img = rng.integers(0, 256, (h0, w0, c) if c > 1 else (h0, w0), dtype=np.uint8)
        dm = rng.random((h0, w0)).astype(np.float32)
        vh, vw = _window(h0, w0)
        wins = [(0, 0, j % 2), ((h0 - vh) // 2, (w0 - vw) // 2, 1 - j % 2), (h0 - vh, w0 - vw, j % 2)]
        if j == len(order) - 2:
            wins[1] = (h0 - vh, w0 - vw, 1 - j % 2)            # the far corner with the other flip as well
        gts = []
        for y0, x0, fl in wins:
            ri, rg = prepare_pair(img[y0:y0 + vh, x0:x0 + vw], dm[y0:y0 + vh, x0:x0 + vw], D, bool(fl))
            pi, pg = np.zeros((3, CH, CW), np.float32), np.zeros((1, CH // D, CW // D), np.float32)
            pi[:, :vh, :vw], pg[:, :vh // D, :vw // D] = ri, rg
            refs.append((pi, pg, vh, vw))
            g = np.zeros((1, CH // D, CW // D), np.float32)
            g[:, :vh // D, :vw // D] = density_to_gt(dm[y0:y0 + vh, x0:x0 + vw], vh, vw, D, bool(fl))
            gts.append(g)
        items.append((torch.from_numpy(img), torch.from_numpy(np.stack(gts)), torch.tensor(wins, dtype=torch.int64)))
    return PackedCollate(crop=(CH, CW))(items), refs


@pytest.fixture(scope="module")
def hand_pack():
    return _hand_pack()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_crop_kernel_matches_cpu_transform(hand_pack, dtype):
    from can_distributed_pytorch_amd.ops.preprocess import preprocess_packed
    packed, refs = hand_pack
    buf, meta = packed
    n, goff = meta[0], meta[3]
    assert n == 15 and meta[5] == 5
    # the last image of the buffer ends (up to the 16-byte alignment) where the ground truth begins, and the last
    # descriptor is its far corner
    last = buf[meta[4]:].view(torch.int64).view(n, 8)[-1].tolist()
    h0, w0, c = SOURCES[-1]
    assert last[1:4] == [h0, w0, c] and last[0] + h0 * w0 * c <= goff < last[0] + h0 * w0 * c + 16
    assert last[5:8] == [h0 - 16, w0 - 24, 1]
    x4, gt = preprocess_packed(packed, "cuda", dtype=dtype)
    torch.cuda.synchronize()
    assert tuple(x4.shape) == (n, CH, CW, 4) and x4.dtype == dtype and tuple(gt.shape) == (n, 1, CH // D, CW // D)
    got = x4.float().cpu().numpy()
    for i, (ri, rg, vh, vw) in enumerate(refs):
        err = np.abs(got[i, ..., :3].transpose(2, 0, 1) - ri).max()
        assert err < 0.03, (i, err)
        assert not got[i, vh:].any() and not got[i, :, vw:].any()          # padding: exact zeros
        assert np.abs(gt[i].cpu().numpy() - rg).max() < 1e-5
    assert not got[..., 3].any()
    # the ground truth is the packed one, bit for bit
    assert torch.equal(gt.cpu().reshape(-1), buf[goff:goff + 4 * gt.numel()].view(torch.float32))


def test_crop_kernel_more_than_one_block_per_sample():
    """A crop of 64 x 96 = 3072 pixel pairs spans 12 blocks per sample; an odd-sized RGB source, flipped."""
    from can_distributed_pytorch_amd.data.transforms import prepare_pair
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, preprocess_packed
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (71, 131, 3), dtype=np.uint8)
    wins = [(7, 35, 1), (0, 0, 0)]
    gts = torch.zeros(2, 1, 8, 12)
    packed = PackedCollate(crop=(64, 96))([(torch.from_numpy(img), gts, torch.tensor(wins))])
    x4, _ = preprocess_packed(packed, "cuda")
    for k, (y0, x0, fl) in enumerate(wins):
        ri, _ = prepare_pair(img[y0:y0 + 64, x0:x0 + 96], np.zeros((64, 96), np.float32), D, bool(fl))
        assert np.abs(x4[k, ..., :3].float().permute(2, 0, 1).cpu().numpy() - ri).max() < 0.03


def test_ahead_prep_matches_preprocess_packed_on_a_cropped_pack(hand_pack):
    from can_distributed_pytorch_amd.ops.preprocess import AheadPrep, preprocess_packed
    packed, _ = hand_pack
    packed2, _ = _hand_pack(order=SOURCES[::-1], seed=4)
    x4, gt = preprocess_packed(packed, "cuda")
    x4b, gtb = preprocess_packed(packed2, "cuda", copy_stream=torch.cuda.Stream("cuda"))
    ap = AheadPrep("cuda")
    h1 = ap.issue(packed)
    h2 = ap.issue(packed2)                                     # a second batch in flight before the first is consumed
    a4, ag = ap.ready(h1)
    b4, bg = ap.ready(h2)
    torch.cuda.synchronize()
    assert torch.equal(a4, x4) and torch.equal(ag, gt)
    assert torch.equal(b4, x4b) and torch.equal(bg, gtb)
    assert not torch.equal(a4, b4)


def test_uncropped_pack_takes_the_unchanged_resize_launch():
    """An uncropped pack through preprocess_packed / AheadPrep == the resize launch called directly."""
    from can_distributed_pytorch_amd.data.dataset import density_to_gt
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops.conv import dt_code
    from can_distributed_pytorch_amd.ops.preprocess import AheadPrep, PackedCollate, preprocess_packed
    C = _ext.require()
    rng = np.random.default_rng(9)
    samples = []
    for i, (h, w, c) in enumerate([(77, 101, 3), (72, 96, 3), (79, 103, 1), (72, 100, 4)]):          # all -> 72 x 96
        img = rng.integers(0, 256, (h, w, c) if c > 1 else (h, w), dtype=np.uint8)
        dm = rng.random((h, w)).astype(np.float32)
        samples.append((torch.from_numpy(img), torch.from_numpy(density_to_gt(dm, h, w, D, bool(i % 2))), bool(i % 2)))
    packed = PackedCollate()(samples)
    buf, (n, ho, wo, goff, doff) = packed
    d = buf.cuda()
    ref = torch.empty(n, ho, wo, 4, dtype=torch.bfloat16, device="cuda")
    C.preprocess_batch(d.data_ptr(), 0, d[doff:].view(torch.int64).data_ptr(), n, ref.data_ptr(), 0, ho, wo, D,
                       dt_code(torch.bfloat16), _ext.stream_ptr(torch.device("cuda")))
    x4, gt = preprocess_packed(packed, "cuda")
    ap = AheadPrep("cuda")
    a4, ag = ap.ready(ap.issue(packed))
    torch.cuda.synchronize()
    assert torch.equal(x4, ref) and torch.equal(a4, ref)
    assert torch.equal(gt.cpu().reshape(-1), buf[goff:goff + 4 * gt.numel()].view(torch.float32)) and torch.equal(ag, gt)


def test_bad_crop_arguments_are_refused_before_any_launch(hand_pack):
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops.preprocess import AheadPrep, PackedCollate, preprocess_packed
    C = _ext.require()
    (buf, meta), _ = hand_pack
    n, doff = meta[0], meta[4]
    canary = torch.full((n, CH, CW, 4), 7.0, dtype=torch.bfloat16, device="cuda")
    d = buf.cuda()

    def launch(host, ch=CH, cw=CW, out=canary):
        C.preprocess_crop(d.data_ptr(), meta[3], d[doff:].view(torch.int64).data_ptr(), host.data_ptr() + doff, n,
                          out.data_ptr(), ch, cw, D, 1, _ext.stream_ptr(torch.device("cuda")))

    # a window that leaves its image (rows 3..5: the 64 x 80 source): one row / one column too far, a negative
    # offset; an image that starts where the packed images end; a descriptor without the crop mark
    for row, slot, value in ((4, 5, 64 - CH + 1), (4, 6, 80 - CW + 1), (0, 5, -1), (14, 0, meta[3]), (2, 7, 0)):
        bad = buf.clone()
        bad[doff:].view(torch.int64).view(n, 8)[row, slot] = value
        with pytest.raises(RuntimeError, match="preprocess_crop"):
            launch(bad)
        if slot in (5, 6):
            for fn in (lambda p: preprocess_packed(p, "cuda"), AheadPrep("cuda").issue):
                with pytest.raises(RuntimeError, match="preprocess_crop"):
                    fn((bad, meta))
    # a crop height of 20 is no multiple of the downsample
    with pytest.raises(RuntimeError, match="preprocess_crop"):
        launch(buf, ch=20)
    with pytest.raises(ValueError):
        PackedCollate(crop=(20, CW))
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all())                         # nothing was launched
    launch(buf)                                                # the same call with the descriptors as packed runs
    torch.cuda.synchronize()
    assert not bool((canary == 7.0).any())


# ---------------------------------------------------------------- train.py end to end
SIZES = [(96, 128), (104, 120), (80, 160), (64, 72), (96, 128), (104, 120)]        # 64 x 72 < the 64 x 96 crop


@pytest.fixture(scope="module")
def jpeg_root(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("crop_jpegs")
    rng = np.random.default_rng(5)
    for split, sizes in (("train_data", SIZES), ("test_data", SIZES[2:4])):
        os.makedirs(root / split / "images")
        os.makedirs(root / split / "ground_truth")
        for i, (h, w) in enumerate(sizes):
            low = rng.integers(0, 256, (h // 8, w // 8, 3), dtype=np.uint8)
            Image.fromarray(low).resize((w, h), Image.BILINEAR).save(root / split / "images" / f"IMG_{i}.jpg", quality=90)
            np.save(root / split / "ground_truth" / f"IMG_{i}.npy", (rng.random((h, w)) * 0.01).astype(np.float32))
    return root


def _train(root, out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--data_root", str(root), "--crop-size", "64x96",
           "--batch-size", "2", "--crops-per-image", "2", "--epochs", "1", "--num-workers", "2", "--wandb", "false",
           "--show", "false", "--log-every", "1", "--init_checkpoint", "", "--seed", "3", "--checkpoint-dir", str(out),
           "--log-jsonl", str(out / "metrics.jsonl"), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(out.parent))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = [json.loads(x) for x in open(out / "metrics.jsonl")]
    return [x for x in recs if x["kind"] == "train"], [x for x in recs if x["kind"] == "epoch"]


def test_train_py_crops_a_mixed_size_jpeg_set(jpeg_root, tmp_path):
    tr, ep = _train(jpeg_root, tmp_path / "a")
    assert [x["step"] for x in tr] == [1, 2, 3]
    assert all(x["input_shape"] == [4, 64, 96, 4] for x in tr)
    assert all(np.isfinite(x["loss"]) and np.isfinite(x["mean_loss"]) for x in tr)
    assert len(ep) == 1 and np.isfinite(ep[0]["loss"]) and np.isfinite(ep[0]["mae"])
    assert ep[0]["eval_batch_size"] == 1 and ep[0]["crop_size"] == [64, 96] and ep[0]["crops_per_image"] == 2
    tr2, _ = _train(jpeg_root, tmp_path / "b")                 # the same seed: the same crops, the same bits
    assert [x["loss"] for x in tr2] == [x["loss"] for x in tr]


def test_train_py_crops_with_graph_and_accumulation(jpeg_root, tmp_path):
    tr, ep = _train(jpeg_root, tmp_path / "g", "--graph", "1", "--accum-steps", "2")
    assert [x["step"] for x in tr] == [1, 2, 3]
    assert all(x["input_shape"] == [4, 64, 96, 4] for x in tr)
    assert tr[0]["loss"] is None and all(np.isfinite(x["loss"]) for x in tr[1:])      # a window closes on step 2
    assert len(ep) == 1 and np.isfinite(ep[0]["loss"]) and ep[0]["eval_batch_size"] == 1
