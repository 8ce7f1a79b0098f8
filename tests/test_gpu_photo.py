"""Photometric jitter on the GPU (csrc/preprocess.hip, the PHOTO kernels behind C.preprocess_crop_photo).

1. Integer-valued tables: the photo launch == the plain launch on images mapped on the host, bit for bit.
2. An identity photo pack == the feature-off pack, bit for bit.
3. Real tables and gray against an fp64 oracle of the definitions (float32 table, float64 taps from _axis_weights).
   Every element: |got - ref| <= ulp16(ref) / 2 + 2^-18 (+ 2^-19 max(sh, sw) for a scaled window), the larger binade's
   ulp where ref is within 2^-18 of a power of two.  2^-18 covers the fp32 lookup, gray, blend and normalise chain; the
   scaled term is lin_tap's fp32 source coordinate (about 3 roundings of 2^-24 src on each of two axes, against a tap
   difference of at most 255 / 255 over sigma_min = 0.224: 27 * 2^-24 max(sh, sw), rounded up).  The worst err / bound
   per kind and dtype is printed with ``pytest -s`` (profiles/r18/photo_errors.txt).
4. One 264 x 1000 sample per kind: more pixel pairs than 512 blocks x 256 threads, so the grid-stride loop runs.
5. AheadPrep == preprocess_packed on photo packs.
6. Bad tables, flags, pointers and descriptors are refused before any launch.
7. train.py --photo-jitter --gray-prob end to end on a generated mixed-size JPEG set.
"""
import functools
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
# anisotropic (sh/CH != sw/CW); placed at (0, 0), in between and at the far corner, in this order.  The unscaled kind
# takes the flips and the places only; its last two images are smaller than the crop (padded)
SOURCES = [((37, 53, 1), [(20, 30, 0), (37, 53, 1), (16, 50, 1)]),
           ((64, 80, 3), [(16, 24, 1), (50, 75, 0), (60, 30, 1)]),
           ((40, 56, 4), [(24, 36, 0), (12, 56, 1), (40, 56, 0)]),
           ((24, 70, 3), [(12, 18, 1), (24, 70, 0), (9, 13, 1)]),
           ((20, 30, 3), [(10, 15, 0), (8, 30, 1), (10, 15, 0), (10, 15, 1)])]
N = sum(len(w) for _, w in SOURCES)
KIND_IDS = ["crop", "crop_scaled", "crop+heads", "crop_scaled+heads"]
KINDS4 = [(False, False), (True, False), (False, True), (True, True)]               # (scaled, heads)
DTYPES = [torch.bfloat16, torch.float16]
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for case, r in _worst.items():
        print(f"\nPHOTO {case:<44s} worst err/bound {r:.4f}", end="")
    if _worst:
        print(f"\nPHOTO worst err / bound over all cases: {max(_worst.values()):.4f}")


def _place(j, h0, w0, sh, sw):
    return [(0, 0), ((h0 - sh) // 2, (w0 - sw) // 2), (h0 - sh, w0 - sw)][min(j, 2)]


def _windows(shape, windows, scaled, crop=(CH, CW)):
    """(y0, x0, flip) or (y0, x0, flip, sh, sw) of every window of one source."""
    h0, w0 = shape[:2]
    out = []
    for j, (sh, sw, fl) in enumerate(windows):
        if not scaled:
            sh, sw = min(crop[0], h0 // D * D), min(crop[1], w0 // D * D)
        out.append(_place(j, h0, w0, sh, sw) + (fl,) + ((sh, sw) if scaled else ()))
    return out


@functools.lru_cache(maxsize=None)
def _scene():
    """Per source: (uint8 image, head records [6, 4], ground truths [K, 1, CH/D, CW/D]); made once, never changed."""
    from can_distributed_pytorch_amd.data.density import heads_table
    rng = np.random.default_rng(3)
    out = []
    for (h0, w0, c), windows in SOURCES:
        img = rng.integers(0, 256, (h0, w0, c) if c > 1 else (h0, w0), dtype=np.uint8)
        heads = heads_table(np.stack([rng.random(6) * w0, rng.random(6) * h0], 1), (h0, w0))
        gts = rng.random((len(windows), 1, CH // D, CW // D)).astype(np.float32)
        out.append((img, np.ascontiguousarray(heads, dtype=np.float32), gts))
    return out


def _items(scaled, heads, rows=None, per_sample_images=None):
    """The items of the SOURCES pack of one kind.  rows [N, 257]: a fourth element per item.  per_sample_images [N]: one
    single-window item per output sample with that image in place of its source (the host-mapped reference)."""
    items, n = [], 0
    for ((h0, w0, c), windows), (img, hd, gts) in zip(SOURCES, _scene()):
        wins = torch.tensor(_windows((h0, w0), windows, scaled), dtype=torch.int64)
        k = len(windows)
        second = torch.from_numpy(hd) if heads else torch.from_numpy(gts)
        if per_sample_images is None:
            item = (torch.from_numpy(img), second, wins)
            items.append(item if rows is None else item + (torch.from_numpy(rows[n:n + k]),))
        else:
            for j in range(k):
                items.append((torch.from_numpy(per_sample_images[n + j]), second if heads else second[j:j + 1],
                              wins[j:j + 1]))
        n += k
    return items


def _collate(scaled, heads, photo):
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate
    return PackedCollate(crop=(CH, CW), crop_scale=scaled, gt_from_heads=heads, photo=photo)


def _sample_sources():
    """[(image, window)] per output sample for both kinds: {scaled: list}."""
    out = {}
    for scaled in (False, True):
        out[scaled] = [(img, w) for ((h0, w0, c), windows), (img, _, _) in zip(SOURCES, _scene())
                       for w in _windows((h0, w0), windows, scaled)]
    return out


def _last_windows_are_the_far_corner(packed, scaled):
    """The last image of the buffer ends (up to the alignment) where the ground truth begins, and the last two
    descriptors are its far corner, unflipped and flipped: a read past the window there leaves the image bytes."""
    buf, meta = packed
    n, goff, doff = meta[0], meta[3], meta[4]
    desc = buf[doff:doff + 64 * n].view(torch.int64).view(n, 8)
    (h0, w0, c), _ = SOURCES[-1]
    eh, ew = (10, 15) if scaled else (16, 24)
    for row, fl in ((desc[-2].tolist(), 0), (desc[-1].tolist(), 1)):
        assert row[1:4] == [h0, w0, c] and row[0] + h0 * w0 * c <= goff < row[0] + h0 * w0 * c + 16
        assert row[4:] == [fl, h0 - eh, w0 - ew, (eh << 32) | ew if scaled else 1]


# ---------------------------------------------------------------- 1. exact: integer tables
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("scaled,heads", KINDS4, ids=KIND_IDS)
def test_integer_tables_equal_the_plain_launch_on_host_mapped_images(scaled, heads, dtype):
    from can_distributed_pytorch_amd.ops.preprocess import _unpack, preprocess_packed
    rng = np.random.default_rng(21)
    maps = rng.integers(0, 256, (N, 256))                       # a random, non-monotone map per sample
    maps[5] = np.arange(256)                                    # one sample with the identity
    assert (np.diff(maps[0]) < 0).any() and len(np.unique(maps[0])) < 256
    rows = np.concatenate([maps.astype(np.float32), np.zeros((N, 1), dtype=np.float32)], 1)
    mapped = [maps[i].astype(np.uint8)[img] for i, (img, _) in enumerate(_sample_sources()[scaled])]
    photo = _collate(scaled, heads, True)(_items(scaled, heads, rows))
    plain = _collate(scaled, heads, False)(_items(scaled, heads, per_sample_images=mapped))
    _last_windows_are_the_far_corner(photo, scaled)
    assert _unpack(photo)[2] == KIND_IDS[KINDS4.index((scaled, heads))] + "+photo" and photo[1][0] == plain[1][0] == N
    a4, ag = preprocess_packed(photo, "cuda", dtype=dtype)
    b4, bg = preprocess_packed(plain, "cuda", dtype=dtype)
    torch.cuda.synchronize()
    assert a4.dtype == b4.dtype == dtype and tuple(a4.shape) == (N, CH, CW, 4)
    assert torch.equal(a4.view(torch.int16), b4.view(torch.int16))
    assert bool((a4[..., :3].float().abs() > 0).any())
    assert torch.equal(ag, bg)                                  # packed, or rendered from the heads by the second launch
    if heads:
        assert bool((ag != 0).any())


# ---------------------------------------------------------------- 2. identity pack == feature off
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("scaled,heads", KINDS4, ids=KIND_IDS)
def test_identity_pack_equals_the_feature_off_pack(scaled, heads, dtype):
    """B = C = 0, G = 1, P = 0: photo_table(0, 1, 1) and no gray for every sample."""
    from can_distributed_pytorch_amd.data.dataset import photo_draw
    from can_distributed_pytorch_amd.data.transforms import photo_table
    from can_distributed_pytorch_amd.ops.preprocess import preprocess_packed
    rows = np.stack([np.concatenate([photo_table(*d[:3]), [np.float32(d[3])]]).astype(np.float32)
                     for d in (photo_draw(3, 1, 0, k, 0.0, 0.0, 1.0, 0.0) for k in range(N))])
    assert np.array_equal(rows[:, :256], np.tile(np.arange(256, dtype=np.float32), (N, 1))) and not rows[:, 256].any()
    on = _collate(scaled, heads, True)(_items(scaled, heads, rows))
    off = _collate(scaled, heads, False)(_items(scaled, heads))
    a4, ag = preprocess_packed(on, "cuda", dtype=dtype)
    b4, bg = preprocess_packed(off, "cuda", dtype=dtype)
    torch.cuda.synchronize()
    assert torch.equal(a4.view(torch.int16), b4.view(torch.int16)) and torch.equal(ag, bg)
    assert bool((a4[..., :3].float().abs() > 0).any())


# ---------------------------------------------------------------- 3. real tables and gray against fp64
def _toned(img, row):
    """fp64 [H, W, 3] on the 0..255 scale: the float32 table looked up, the gray mix with the float32 coefficients."""
    t = row[:256].astype(np.float64)[img.reshape(img.shape[0], img.shape[1], -1)]
    if t.shape[2] == 1:
        return np.repeat(t, 3, axis=2)                          # gray is ignored for one channel
    t = t[..., :3]
    if row[256]:
        w = np.array([0.299, 0.587, 0.114], dtype=np.float32).astype(np.float64)
        y = w[2] * t[..., 2] + (w[1] * t[..., 1] + w[0] * t[..., 0])
        t = np.stack([y, y, y], axis=2)
    return t


def _oracle(img, row, win, crop=(CH, CW)):
    """(ref fp64 [ch, cw, 3], valid bool [ch, cw], pre-normalisation values [ch, cw, 3]) of one output sample."""
    from can_distributed_pytorch_amd.data.transforms import _axis_weights
    ch, cw = crop
    t = _toned(img, row)
    valid = np.ones((ch, cw), dtype=bool)
    if len(win) == 5:
        y0, x0, fl, sh, sw = win
        w = t[y0:y0 + sh, x0:x0 + sw]
        w = w[:, ::-1] if fl else w                             # the flip comes before the resample
        ya, yb, fy = _axis_weights(sh, ch)
        xa, xb, fx = _axis_weights(sw, cw)
        r = w[ya] * (1.0 - fy)[:, None, None] + w[yb] * fy[:, None, None]
        p = r[:, xa] * (1.0 - fx)[None, :, None] + r[:, xb] * fx[None, :, None]
    else:
        y0, x0, fl = win
        vh, vw = min(ch, img.shape[0] // D * D), min(cw, img.shape[1] // D * D)
        w = t[y0:y0 + vh, x0:x0 + vw]
        p = np.zeros((ch, cw, 3))
        p[:vh, :vw] = w[:, ::-1] if fl else w
        valid[vh:] = False
        valid[:, vw:] = False
    ref = (p / 255.0 - MEAN) / STD
    ref[~valid] = 0.0                                           # the padding is not jittered: it stays zero
    return ref, valid, p


def _bound(ref, dtype, extra=0.0):
    """ulp16(ref) / 2 + 2^-18 + extra, the larger binade's ulp where ref is within 2^-18 of a power of two."""
    a = np.abs(ref)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -60)))
    e = np.where(2.0 ** (e + 1) - a <= 2.0 ** -18, e + 1, e)
    ulp = 2.0 ** (np.maximum(e, -14.0) - 10) if dtype == torch.float16 else 2.0 ** (e - 7)
    return ulp / 2 + 2.0 ** -18 + extra


def _check(case, x4, samples, rows, dtype, crop=(CH, CW)):
    """Every element of x4 [n, ch, cw, 4] against the oracle; the padding and channel 3 are zero bits."""
    bits = x4.view(torch.int16).cpu().numpy()
    got = x4.float().cpu().numpy().astype(np.float64)
    assert not bits[..., 3].any()
    worst = 0.0
    for i, ((img, win), row) in enumerate(zip(samples, rows)):
        ref, valid, p = _oracle(img, row, win, crop)
        if row[256] and img.ndim == 3:                          # a gray sample: three equal values before normalisation
            assert np.array_equal(p[..., 0], p[..., 1]) and np.array_equal(p[..., 0], p[..., 2])
        assert not bits[i][~valid].any(), f"{case}: sample {i}: padding is not zero"
        extra = 2.0 ** -19 * max(win[3], win[4]) if len(win) == 5 else 0.0
        ratio = np.abs(got[i, ..., :3] - ref)[valid] / _bound(ref, dtype, extra)[valid]
        worst = max(worst, float(ratio.max()))
    _worst[case] = worst
    print(f"PHOTO {case}: worst err / bound {worst:.4f}")
    assert worst <= 1.0, f"{case}: err / bound = {worst:.4g}"


@functools.lru_cache(maxsize=None)
def _real_rows(n, seed):
    """[n, 257]: tables over the whole accepted range of (b, c, g), every second sample gray."""
    from can_distributed_pytorch_amd.data.transforms import photo_table
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 257), dtype=np.float32)
    for i in range(n):
        rows[i, :256] = photo_table(rng.uniform(-0.5, 0.5), 2.0 ** rng.uniform(-1, 1), 2.0 ** rng.uniform(-1, 1))
        rows[i, 256] = i % 2
    rows[0, :256] = photo_table(0.5, 2.0, 0.5)                  # the corners of the range: clipped at both ends
    rows[1, :256] = photo_table(-0.5, 2.0, 2.0)
    return rows


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("scaled", [False, True], ids=["crop", "crop_scaled"])
def test_real_tables_and_gray_against_fp64(scaled, dtype):
    from can_distributed_pytorch_amd.ops.preprocess import preprocess_packed
    rows = _real_rows(N, 31)
    gray = [i for i in range(N) if rows[i, 256]]
    chans = {_sample_sources()[scaled][i][0].shape[2:] for i in gray}
    assert chans == {(), (3,), (4,)}                            # gray samples of 1, 3 and 4 channels
    packed = _collate(scaled, False, True)(_items(scaled, False, rows))
    _last_windows_are_the_far_corner(packed, scaled)
    x4, _ = preprocess_packed(packed, "cuda", dtype=dtype)
    torch.cuda.synchronize()
    _check(f"{KIND_IDS[scaled]} {CH}x{CW} {str(dtype)[6:]}", x4, _sample_sources()[scaled], rows, dtype)


# ---------------------------------------------------------------- 4. the grid-stride loop
BIG = (264, 1000)                                               # 132000 pixel pairs > 512 blocks x 256 threads


@functools.lru_cache(maxsize=None)
def _big(scaled):
    """One sample: unscaled, an image smaller than the crop (padded); scaled, a shrunk-and-magnified flipped window."""
    rng = np.random.default_rng(41 + scaled)
    img = rng.integers(0, 256, (203, 907, 3) if not scaled else (150, 1300, 3), dtype=np.uint8)
    win = (3, 3, 1) if not scaled else (7, 30, 1, 140, 1250)    # the unscaled one: the far corner of 203 x 907
    row = _real_rows(2, 43)[scaled:scaled + 1].copy()
    row[0, 256] = scaled
    gts = torch.zeros(1, 1, BIG[0] // D, BIG[1] // D)
    return (torch.from_numpy(img), gts, torch.tensor([win], dtype=torch.int64), torch.from_numpy(row)), img, win, row


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("scaled", [False, True], ids=["crop", "crop_scaled"])
def test_one_large_sample_runs_the_grid_stride_loop(scaled, dtype):
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, preprocess_packed
    item, img, win, row = _big(scaled)
    assert BIG[0] * (BIG[1] // 2) > 512 * 256
    packed = PackedCollate(crop=BIG, crop_scale=scaled, photo=True)([item])
    x4, _ = preprocess_packed(packed, "cuda", dtype=dtype)
    torch.cuda.synchronize()
    assert tuple(x4.shape) == (1, *BIG, 4)
    if not scaled:                                              # 200 x 904 valid, the rest padding: zero in all channels
        bits = x4.view(torch.int16)
        assert not bool(bits[0, 200:].any()) and not bool(bits[0, :, 904:].any()) and bool(bits[0, :200, :904, :3].any())
    _check(f"{KIND_IDS[scaled]} {BIG[0]}x{BIG[1]} {str(dtype)[6:]}", x4, [(img, win)], row, dtype, BIG)


# ---------------------------------------------------------------- 5. AheadPrep
def test_ahead_prep_matches_preprocess_packed_on_photo_packs():
    from can_distributed_pytorch_amd.ops.preprocess import AheadPrep, PackedCollate, preprocess_packed
    rows = _real_rows(N, 31)
    packed = _collate(True, True, True)(_items(True, True, rows))
    packed2 = PackedCollate(crop=BIG, photo=True)([_big(False)[0]])
    x4, gt = preprocess_packed(packed, "cuda")
    x4b, gtb = preprocess_packed(packed2, "cuda", copy_stream=torch.cuda.Stream("cuda"))
    ap = AheadPrep("cuda")
    h1 = ap.issue(packed)
    h2 = ap.issue(packed2)                                     # a second batch in flight before the first is consumed
    a4, ag = ap.ready(h1)
    b4, bg = ap.ready(h2)
    torch.cuda.synchronize()
    assert torch.equal(a4, x4) and torch.equal(ag, gt) and bool((gt != 0).any())
    assert torch.equal(b4, x4b) and torch.equal(bg, gtb)
    assert a4.shape != b4.shape


# ---------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("scaled", [False, True], ids=["crop", "crop_scaled"])
def test_bad_photo_packs_are_refused_before_any_launch(scaled):
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops.conv import dt_code
    from can_distributed_pytorch_amd.ops.preprocess import AheadPrep, preprocess_packed
    C = _ext.require()
    buf, meta = _collate(scaled, False, True)(_items(scaled, False, _real_rows(N, 31)))
    n, goff, doff, poff = meta[0], meta[3], meta[4], meta[8]
    canary = torch.full((n, CH, CW, 4), 7.0, dtype=torch.bfloat16, device="cuda")
    d = buf.cuda()
    st = _ext.stream_ptr(torch.device("cuda"))

    def launch(host, shift=0):
        C.preprocess_crop_photo(d.data_ptr(), goff, d.data_ptr() + doff, host.data_ptr() + doff, n, canary.data_ptr(),
                                CH, CW, D, dt_code(torch.bfloat16), st, d.data_ptr() + poff + shift,
                                host.data_ptr() + poff + shift, int(scaled))

    def edited(region, row, slot, value):
        bad = buf.clone()
        if region == "photo":
            bad[poff:].view(torch.float32).view(n, 260)[row, slot] = value
        else:
            bad[doff:doff + 64 * n].view(torch.int64).view(n, 8)[row, slot] = value
        return bad

    bad_packs = [edited("photo", 0, 0, float("nan")), edited("photo", n - 1, 255, float("nan")),
                 edited("photo", 3, 17, 255.5), edited("photo", 3, 17, float("inf")), edited("photo", 7, 200, -1.0),
                 edited("photo", 2, 256, 0.5), edited("photo", n - 1, 256, 2.0), edited("photo", 1, 256, float("nan")),
                 edited("desc", 4, 5, 64), edited("desc", 1, 3, 2), edited("desc", 0, 7, 0)]      # bad descriptors
    for bad in bad_packs:
        with pytest.raises(RuntimeError, match="preprocess_crop_photo"):
            launch(bad)
        for fn in (lambda p: preprocess_packed(p, "cuda"), AheadPrep("cuda").issue):
            with pytest.raises(RuntimeError, match="preprocess_crop_photo"):
                fn((bad, meta))
    for shift in (4, 8):                                       # a photo pointer off 16 bytes; a null one
        with pytest.raises(RuntimeError, match="preprocess_crop_photo"):
            launch(buf, shift)
    with pytest.raises(RuntimeError, match="preprocess_crop_photo"):
        C.preprocess_crop_photo(d.data_ptr(), goff, d.data_ptr() + doff, buf.data_ptr() + doff, n, canary.data_ptr(),
                                CH, CW, D, dt_code(torch.bfloat16), st, 0, buf.data_ptr() + poff, int(scaled))
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all())                         # nothing was launched
    launch(buf)                                                # the same call with the pack as packed runs
    torch.cuda.synchronize()
    assert not bool((canary == 7.0).any())


# ---------------------------------------------------------------- 7. train.py end to end
SIZES = [(96, 128), (104, 120), (80, 160), (64, 72), (96, 128), (104, 120)]


@pytest.fixture(scope="module")
def jpeg_root(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("photo_jpegs")
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
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--data_root", str(root), "--crop-size", "64x64",
           "--crop-scale", "0.75,1.33", "--photo-jitter", "0.2,0.3,1.5", "--gray-prob", "0.3", "--batch-size", "2",
           "--crops-per-image", "2", "--epochs", "1", "--num-workers", "2", "--wandb", "false", "--show", "false",
           "--log-every", "1", "--init_checkpoint", "", "--seed", "3", "--checkpoint-dir", str(out),
           "--log-jsonl", str(out / "metrics.jsonl"), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(out.parent))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = [json.loads(x) for x in open(out / "metrics.jsonl")]
    return [x for x in recs if x["kind"] == "train"], [x for x in recs if x["kind"] == "epoch"]


def test_train_py_photo_jitter_on_a_mixed_size_jpeg_set(jpeg_root, tmp_path):
    tr, ep = _train(jpeg_root, tmp_path / "a")
    assert [x["step"] for x in tr] == [1, 2, 3]
    assert all(x["input_shape"] == [4, 64, 64, 4] for x in tr)
    assert all(np.isfinite(x["loss"]) and np.isfinite(x["mean_loss"]) for x in tr)
    assert len(ep) == 1 and np.isfinite(ep[0]["loss"]) and np.isfinite(ep[0]["mae"])
    assert ep[0]["crop_size"] == [64, 64] and ep[0]["crop_scale"] == [0.75, 1.33]
    assert ep[0]["photo_jitter"] == [0.2, 0.3, 1.5] and ep[0]["gray_prob"] == 0.3


def test_train_py_photo_jitter_with_graph_and_accumulation(jpeg_root, tmp_path):
    tr, ep = _train(jpeg_root, tmp_path / "g", "--graph", "1", "--accum-steps", "2")
    assert [x["step"] for x in tr] == [1, 2, 3]
    assert all(x["input_shape"] == [4, 64, 64, 4] for x in tr)
    assert tr[0]["loss"] is None and all(np.isfinite(x["loss"]) for x in tr[1:])      # a window closes on step 2
    assert len(ep) == 1 and np.isfinite(ep[0]["loss"]) and np.isfinite(ep[0]["mae"])
    assert ep[0]["photo_jitter"] == [0.2, 0.3, 1.5] and ep[0]["gray_prob"] == 0.3
