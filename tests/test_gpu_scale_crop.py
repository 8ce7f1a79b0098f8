"""Random-scale crops on the GPU: the scaled crop kernel against prepare_pair_scaled on the window's slices, unit
windows against the unscaled crop kernel bit for bit, the scaled pack through preprocess_packed / AheadPrep, refused
descriptors, the untouched unscaled launches, and train.py --crop-scale end to end on a generated mixed-size JPEG
set."""
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
# per source (H0, W0, C): windows (sh, sw, flip) -- magnified (sh < CH), shrunk (sh > CH, where the image allows) and
# anisotropic (sh/CH != sw/CW); placed at (0, 0), in between and at the far corner, in this order
SOURCES = [((37, 53, 1), [(20, 30, 0), (37, 53, 1), (16, 50, 1)]),
           ((64, 80, 3), [(16, 24, 1), (50, 75, 0), (60, 30, 1)]),
           ((40, 56, 4), [(24, 36, 0), (12, 56, 1), (40, 56, 0)]),
           ((24, 70, 3), [(12, 18, 1), (24, 70, 0), (9, 13, 1)]),
           ((20, 30, 3), [(10, 15, 0), (8, 30, 1), (10, 15, 0), (10, 15, 1)])]


def _place(j, h0, w0, sh, sw):
    return [(0, 0), ((h0 - sh) // 2, (w0 - sw) // 2), (h0 - sh, w0 - sw)][min(j, 2)]


def _hand_pack(sources=SOURCES, seed=3, crop=(CH, CW)):
    """A scaled pack built by hand.  The LAST two descriptors are the far corner of the last image of the buffer,
    unflipped and flipped: a read past the window there lands in the ground truth bytes.  Returns (packed, refs) with
    refs[n] = prepare_pair_scaled's image of output sample n."""
    from can_distributed_pytorch_amd.data.dataset import density_to_gt_scaled
    from can_distributed_pytorch_amd.data.transforms import prepare_pair_scaled
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate
    rng = np.random.default_rng(seed)
    ch, cw = crop
    items, refs = [], []
    for (h0, w0, c), windows in sources:
        img = rng.integers(0, 256, (h0, w0, c) if c > 1 else (h0, w0), dtype=np.uint8)
        dm = rng.random((h0, w0)).astype(np.float32)
        wins, gts = [], []
        for j, (sh, sw, fl) in enumerate(windows):
            y0, x0 = _place(j, h0, w0, sh, sw)
            wins.append((y0, x0, fl, sh, sw))
            ri, rg = prepare_pair_scaled(img[y0:y0 + sh, x0:x0 + sw], dm[y0:y0 + sh, x0:x0 + sw], ch, cw, D, bool(fl))
            g = density_to_gt_scaled(dm[y0:y0 + sh, x0:x0 + sw], ch, cw, D, bool(fl))
            assert g.tobytes() == rg.tobytes()
            refs.append(ri)
            gts.append(g)
        items.append((torch.from_numpy(img), torch.from_numpy(np.stack(gts)), torch.tensor(wins, dtype=torch.int64)))
    return PackedCollate(crop=crop, crop_scale=True)(items), refs


@pytest.fixture(scope="module")
def hand_pack():
    return _hand_pack()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_scaled_kernel_matches_cpu_transform(hand_pack, dtype):
    from can_distributed_pytorch_amd.ops.preprocess import preprocess_packed
    packed, refs = hand_pack
    buf, meta = packed
    n, goff, doff = meta[0], meta[3], meta[4]
    assert n == 16 and meta[5:] == (5, 1)
    # the last image of the buffer ends (up to the 16-byte alignment) where the ground truth begins, and the last two
    # descriptors are its far corner, unflipped and flipped
    desc = buf[doff:].view(torch.int64).view(n, 8)
    (h0, w0, c), _ = SOURCES[-1]
    for row, fl in ((desc[-2].tolist(), 0), (desc[-1].tolist(), 1)):
        assert row[1:4] == [h0, w0, c] and row[0] + h0 * w0 * c <= goff < row[0] + h0 * w0 * c + 16
        assert row[4:] == [fl, h0 - 10, w0 - 15, (10 << 32) | 15]
    x4, gt = preprocess_packed(packed, "cuda", dtype=dtype)
    torch.cuda.synchronize()
    assert tuple(x4.shape) == (n, CH, CW, 4) and x4.dtype == dtype and tuple(gt.shape) == (n, 1, CH // D, CW // D)
    got = x4.float().cpu().numpy()
    errs = [float(np.abs(got[i, ..., :3].transpose(2, 0, 1) - ri).max()) for i, ri in enumerate(refs)]
    print("max |kernel - prepare_pair_scaled| per sample:", " ".join(f"{e:.4f}" for e in errs))
    assert max(errs) < 0.03, errs
    assert not got[..., 3].any()
    # the ground truth is the packed one, bit for bit
    assert torch.equal(gt.cpu().reshape(-1), buf[goff:goff + 4 * gt.numel()].view(torch.float32))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_unit_windows_equal_the_unscaled_crop_kernel_bit_for_bit(dtype):
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, preprocess_packed
    rng = np.random.default_rng(6)
    plain, scaled = [], []
    for j, (h0, w0, c) in enumerate([(37, 53, 1), (64, 80, 3), (40, 56, 4), (32, 48, 3)]):
        img = torch.from_numpy(rng.integers(0, 256, (h0, w0, c) if c > 1 else (h0, w0), dtype=np.uint8))
        wins = [(0, 0, j % 2), ((h0 - CH) // 2, (w0 - CW) // 2, 1 - j % 2), (h0 - CH, w0 - CW, j % 2)]
        gts = torch.from_numpy(rng.random((3, 1, CH // D, CW // D)).astype(np.float32))
        plain.append((img, gts, torch.tensor(wins, dtype=torch.int64)))
        scaled.append((img, gts, torch.tensor([w + (CH, CW) for w in wins], dtype=torch.int64)))
    a4, ag = preprocess_packed(PackedCollate(crop=(CH, CW))(plain), "cuda", dtype=dtype)
    b4, bg = preprocess_packed(PackedCollate(crop=(CH, CW), crop_scale=True)(scaled), "cuda", dtype=dtype)
    torch.cuda.synchronize()
    assert a4.dtype == b4.dtype == dtype and torch.equal(a4.view(torch.int16), b4.view(torch.int16))
    assert torch.equal(ag, bg)
    assert bool((a4[..., :3].float().abs() > 0).any())


def test_scaled_kernel_more_than_one_block_per_sample():
    """A crop of 64 x 96 = 3072 pixel pairs spans 12 blocks per sample; an odd-sized RGB source, shrunk and flipped."""
    sources = [((71, 131, 3), [(70, 120, 0), (66, 99, 1), (71, 131, 1)])]
    packed, refs = _hand_pack(sources, seed=8, crop=(64, 96))
    from can_distributed_pytorch_amd.ops.preprocess import preprocess_packed
    x4, _ = preprocess_packed(packed, "cuda")
    assert tuple(x4.shape) == (3, 64, 96, 4)
    got = x4.float().cpu().numpy()
    for k, ri in enumerate(refs):
        assert np.abs(got[k, ..., :3].transpose(2, 0, 1) - ri).max() < 0.03
    assert not got[..., 3].any()


def test_ahead_prep_matches_preprocess_packed_on_a_scaled_pack(hand_pack):
    from can_distributed_pytorch_amd.ops.preprocess import AheadPrep, preprocess_packed
    packed, _ = hand_pack
    packed2, _ = _hand_pack(SOURCES[:4][::-1], seed=4)
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
    assert a4.shape != b4.shape


def test_bad_scaled_descriptors_are_refused_before_any_launch():
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops.preprocess import AheadPrep, preprocess_packed
    C = _ext.require()
    # rows 0..2: the 140 x 200 gray source (large enough for a window beyond 4 x the crop), rows 3..5: 64 x 80 RGB
    sources = [((140, 200, 1), [(40, 60, 0), (100, 150, 1), (128, 192, 0)]),
               ((64, 80, 3), [(16, 24, 1), (50, 75, 0), (60, 30, 1)])]
    (buf, meta), _ = _hand_pack(sources, seed=5)
    n, goff, doff = meta[0], meta[3], meta[4]
    canary = torch.full((n, CH, CW, 4), 7.0, dtype=torch.bfloat16, device="cuda")
    d = buf.cuda()
    st = _ext.stream_ptr(torch.device("cuda"))

    def launch(host, ch=CH, cw=CW, ds=D):
        C.preprocess_crop_scaled(d.data_ptr(), goff, d[doff:].view(torch.int64).data_ptr(), host.data_ptr() + doff, n,
                                 canary.data_ptr(), ch, cw, ds, 1, st)

    ext = lambda sh, sw: (sh << 32) | sw
    bad_fields = [
        (4, 5, 64 - 50 + 1), (4, 6, 80 - 75 + 1), (3, 5, -1), (3, 6, -1),          # a window past its image
        (3, 7, ext(0, 24)), (3, 7, ext(16, 0)), (3, 7, ext(65, 24)), (3, 7, ext(16, 81)),      # empty / larger than it
        (0, 7, ext(129, 60)), (0, 7, ext(40, 193)), (3, 7, ext(7, 24)), (3, 7, ext(16, 11)),  # beyond 4x either way
        (2, 7, 1), (5, 7, 0), (0, 7, -1),                      # the unscaled mark, no mark
        (5, 0, goff), (5, 0, goff - 64 * 80 * 3 + 1), (0, 0, -1),                  # an image past the packed bytes
        (1, 3, 2), (1, 4, 2), (0, 1, 0),                       # what the unscaled entry refuses too
    ]
    for row, slot, value in bad_fields:
        bad = buf.clone()
        bad[doff:].view(torch.int64).view(n, 8)[row, slot] = value
        with pytest.raises(RuntimeError, match="preprocess_crop_scaled"):
            launch(bad)
        for fn in (lambda p: preprocess_packed(p, "cuda"), AheadPrep("cuda").issue):
            with pytest.raises(RuntimeError, match="preprocess_crop_scaled"):
                fn((bad, meta))
    # an odd crop width (downsample 1, so that nothing else is wrong with it); a height that is no multiple of 8
    for kw in (dict(cw=47, ds=1), dict(ch=20)):
        with pytest.raises(RuntimeError, match="preprocess_crop_scaled"):
            launch(buf, **kw)
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all())                         # nothing was launched
    launch(buf)                                                # the same call with the descriptors as packed runs
    torch.cuda.synchronize()
    assert not bool((canary == 7.0).any())


def test_unscaled_packs_take_their_unchanged_launches():
    """An unscaled cropped pack and an uncropped pack through preprocess_packed / AheadPrep == C.preprocess_crop and
    C.preprocess_batch called directly."""
    from can_distributed_pytorch_amd.data.dataset import density_to_gt
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops.conv import dt_code
    from can_distributed_pytorch_amd.ops.preprocess import AheadPrep, PackedCollate, preprocess_packed
    C = _ext.require()
    st = _ext.stream_ptr(torch.device("cuda"))
    rng = np.random.default_rng(9)
    # cropped, unscaled: one image as large as needed, one smaller than the crop (padded)
    items = []
    for h0, w0, c in [(64, 80, 3), (20, 30, 3), (37, 53, 1)]:
        img = rng.integers(0, 256, (h0, w0, c) if c > 1 else (h0, w0), dtype=np.uint8)
        vh, vw = min(CH, h0 // D * D), min(CW, w0 // D * D)
        wins = [(0, 0, 1), (h0 - vh, w0 - vw, 0)]
        gts = torch.from_numpy(rng.random((2, 1, CH // D, CW // D)).astype(np.float32))
        items.append((torch.from_numpy(img), gts, torch.tensor(wins, dtype=torch.int64)))
    packed = PackedCollate(crop=(CH, CW))(items)
    buf, meta = packed
    n, goff, doff = meta[0], meta[3], meta[4]
    assert len(meta) == 6
    d = buf.cuda()
    ref = torch.empty(n, CH, CW, 4, dtype=torch.bfloat16, device="cuda")
    C.preprocess_crop(d.data_ptr(), goff, d[doff:].view(torch.int64).data_ptr(), buf.data_ptr() + doff, n,
                      ref.data_ptr(), CH, CW, D, dt_code(torch.bfloat16), st)
    x4, gt = preprocess_packed(packed, "cuda")
    ap = AheadPrep("cuda")
    a4, ag = ap.ready(ap.issue(packed))
    torch.cuda.synchronize()
    assert torch.equal(x4, ref) and torch.equal(a4, ref) and torch.equal(ag, gt)
    assert torch.equal(gt.cpu().reshape(-1), buf[goff:goff + 4 * gt.numel()].view(torch.float32))
    # uncropped: the resize launch
    samples = []
    for i, (h, w, c) in enumerate([(77, 101, 3), (72, 96, 3), (79, 103, 1)]):          # all -> 72 x 96
        img = rng.integers(0, 256, (h, w, c) if c > 1 else (h, w), dtype=np.uint8)
        dm = rng.random((h, w)).astype(np.float32)
        samples.append((torch.from_numpy(img), torch.from_numpy(density_to_gt(dm, h, w, D, bool(i % 2))), bool(i % 2)))
    packed = PackedCollate()(samples)
    buf, (n, ho, wo, goff, doff) = packed
    d = buf.cuda()
    ref = torch.empty(n, ho, wo, 4, dtype=torch.bfloat16, device="cuda")
    C.preprocess_batch(d.data_ptr(), 0, d[doff:].view(torch.int64).data_ptr(), n, ref.data_ptr(), 0, ho, wo, D,
                       dt_code(torch.bfloat16), st)
    x4, gt = preprocess_packed(packed, "cuda")
    a4, ag = ap.ready(ap.issue(packed))
    torch.cuda.synchronize()
    assert torch.equal(x4, ref) and torch.equal(a4, ref) and torch.equal(ag, gt)


# ---------------------------------------------------------------- the launches against one another
def _uncropped_pack(shapes, seed):
    """An uncropped pack of random images of the given (H, W, C), flips alternating, zero ground truths."""
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate
    rng = np.random.default_rng(seed)
    h, w = shapes[0][0] // D * D, shapes[0][1] // D * D
    gt = torch.zeros(1, h // D, w // D)
    return PackedCollate()([(torch.from_numpy(rng.integers(0, 256, (h0, w0, c) if c > 1 else (h0, w0), dtype=np.uint8)),
                             gt, bool(i % 2)) for i, (h0, w0, c) in enumerate(shapes)])


def _resize_launch(C, d, n, doff, ho, wo, dtype):
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops.conv import dt_code
    out = torch.empty(n, ho, wo, 4, dtype=dtype, device="cuda")
    C.preprocess_batch(d.data_ptr(), 0, d[doff:].view(torch.int64).data_ptr(), n, out.data_ptr(), 0, ho, wo, D,
                       dt_code(dtype), _ext.stream_ptr(torch.device("cuda")))
    return out


# the second case: 128 x 64 = 4096 pixel pairs, so a sample spans more than one block of either launch
@pytest.mark.parametrize("shapes", [[(77, 101, 3), (72, 96, 3), (79, 103, 1), (72, 100, 4)], [(131, 71, 3)]],
                         ids=["to72x96", "to128x64"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_resize_launch_equals_scaled_launch_on_whole_image_windows(shapes, dtype):
    """C.preprocess_batch on an uncropped pack == C.preprocess_crop_scaled on the same bytes with every window set
    to its whole image, bit for bit: what lets one resample kernel serve both entries."""
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops.conv import dt_code
    C = _ext.require()
    buf, (n, ho, wo, goff, doff) = _uncropped_pack(shapes, seed=12)
    d = buf.cuda()
    a4 = _resize_launch(C, d, n, doff, ho, wo, dtype)
    whole = buf.clone()
    rows = whole[doff:].view(torch.int64).view(n, 8)
    assert rows[:, 4].tolist() == [i % 2 for i in range(n)] and not rows[:, 5:].any()
    rows[:, 7] = (rows[:, 1] << 32) | rows[:, 2]
    dw = whole.cuda()
    b4 = torch.empty_like(a4)
    C.preprocess_crop_scaled(dw.data_ptr(), goff, dw[doff:].view(torch.int64).data_ptr(), whole.data_ptr() + doff, n,
                             b4.data_ptr(), ho, wo, D, dt_code(dtype), _ext.stream_ptr(torch.device("cuda")))
    torch.cuda.synchronize()
    assert (ho, wo) == ((72, 96) if n == 4 else (128, 64))
    assert torch.equal(a4.view(torch.int16), b4.view(torch.int16))
    assert bool((a4[..., :3].float().abs() > 0).any())


@pytest.mark.parametrize("shape", [(77, 101, 3), (50, 70, 1)])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_per_sample_form_equals_the_batch_launch_bit_for_bit(shape, flip, dtype):
    """preprocess_batch (C.preprocess_image + C.preprocess_density per sample) against the batch launch on the same
    single image, bit for bit.  The batch launch resizes images only: its density half had no caller, equalled
    C.preprocess_density bit for bit when it was deleted (profiles/r14), and C.preprocess_density stays held to the
    CPU transform by tests/test_gpu_components.py."""
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, preprocess_batch
    C = _ext.require()
    h0, w0, c = shape
    rng = np.random.default_rng(13)
    img = torch.from_numpy(rng.integers(0, 256, (h0, w0, c) if c > 1 else (h0, w0), dtype=np.uint8))
    dm = torch.from_numpy(rng.random((h0, w0)).astype(np.float32))
    buf, (n, ho, wo, goff, doff) = PackedCollate()([(img, torch.zeros(1, h0 // D, w0 // D), flip)])
    a4 = _resize_launch(C, buf.cuda(), n, doff, ho, wo, dtype)
    x4, gt = preprocess_batch([img], [dm], [flip], "cuda", dtype=dtype)
    torch.cuda.synchronize()
    assert x4.dtype == dtype and torch.equal(a4.view(torch.int16), x4.view(torch.int16))
    assert bool((x4[..., :3].float().abs() > 0).any())
    assert tuple(gt.shape) == (1, 1, h0 // D, w0 // D) and bool(torch.isfinite(gt).all())


def test_resize_launch_refuses_densities_before_any_launch():
    """C.preprocess_batch resizes images only: a non-null density or ground-truth pointer is refused."""
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops.conv import dt_code
    C = _ext.require()
    buf, (n, ho, wo, goff, doff) = _uncropped_pack([(77, 101, 3), (72, 96, 3)], seed=14)
    d = buf.cuda()
    st = _ext.stream_ptr(torch.device("cuda"))
    canary = torch.full((n, ho, wo, 4), 7.0, dtype=torch.bfloat16, device="cuda")
    dens = torch.zeros(77 * 101 + 72 * 96, device="cuda")
    gt = torch.full((n, 1, ho // D, wo // D), 7.0, device="cuda")
    for dp, gp in ((dens.data_ptr(), gt.data_ptr()), (dens.data_ptr(), 0), (0, gt.data_ptr())):
        with pytest.raises(RuntimeError, match="preprocess_batch"):
            C.preprocess_batch(d.data_ptr(), dp, d[doff:].view(torch.int64).data_ptr(), n, canary.data_ptr(), gp, ho,
                               wo, D, dt_code(torch.bfloat16), st)
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all()) and bool((gt == 7.0).all())          # nothing was launched
    C.preprocess_batch(d.data_ptr(), 0, d[doff:].view(torch.int64).data_ptr(), n, canary.data_ptr(), 0, ho, wo, D,
                       dt_code(torch.bfloat16), st)
    torch.cuda.synchronize()
    assert not bool((canary == 7.0).any())


# ---------------------------------------------------------------- train.py end to end
SIZES =[(96, 128), (104, 120), (80, 160), (64, 72), (96, 128), (104, 120)]        # 64 x 72 < the 64 x 96 crop


@pytest.fixture(scope="module")
def jpeg_root(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("scale_jpegs")
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
           "--crop-scale", "0.75,1.33", "--batch-size", "2", "--crops-per-image", "2", "--epochs", "1",
           "--num-workers", "2", "--wandb", "false", "--show", "false", "--log-every", "1", "--init_checkpoint", "",
           "--seed", "3", "--checkpoint-dir", str(out), "--log-jsonl", str(out / "metrics.jsonl"), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(out.parent))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = [json.loads(x) for x in open(out / "metrics.jsonl")]
    return [x for x in recs if x["kind"] == "train"], [x for x in recs if x["kind"] == "epoch"]


def test_train_py_scaled_crops_of_a_mixed_size_jpeg_set(jpeg_root, tmp_path):
    tr, ep = _train(jpeg_root, tmp_path / "a")
    assert [x["step"] for x in tr] == [1, 2, 3]
    assert all(x["input_shape"] == [4, 64, 96, 4] for x in tr)
    assert all(np.isfinite(x["loss"]) and np.isfinite(x["mean_loss"]) for x in tr)
    assert len(ep) == 1 and np.isfinite(ep[0]["loss"]) and np.isfinite(ep[0]["mae"])
    assert ep[0]["eval_batch_size"] == 1 and ep[0]["crop_size"] == [64, 96] and ep[0]["crop_scale"] == [0.75, 1.33]


def test_train_py_scaled_crops_with_graph_and_accumulation(jpeg_root, tmp_path):
    tr, ep = _train(jpeg_root, tmp_path / "g", "--graph", "1", "--accum-steps", "2")
    assert [x["step"] for x in tr] == [1, 2, 3]
    assert all(x["input_shape"] == [4, 64, 96, 4] for x in tr)
    assert tr[0]["loss"] is None and all(np.isfinite(x["loss"]) for x in tr[1:])      # a window closes on step 2
    assert len(ep) == 1 and np.isfinite(ep[0]["loss"]) and ep[0]["eval_batch_size"] == 1
