"""Photometric jitter on the CPU: the stateless photo draw, the tone table, apply_photo, CrowdDataset(photo_jitter=,
gray_prob=) items, the photo region of PackedCollate packs of all four cropped kinds, and the train.py options."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from can_distributed_pytorch_amd.data import dataset as DS
from can_distributed_pytorch_amd.data.dataset import (CrowdDataset, _as_uint8, crop_draw, crop_window, photo_draw,
                                                      scale_draw, scaled_window)
from can_distributed_pytorch_amd.data.density import gaussian_filter_density, heads_path, heads_table
from can_distributed_pytorch_amd.data.transforms import (apply_photo, gray_to_rgb, photo_table, prepare_pair,
                                                         prepare_pair_scaled, to_unit_float)
from can_distributed_pytorch_amd.ops.preprocess import PackedCollate, _unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BCGP = (0.2, 0.3, 1.5, 0.3)
CROP, D, K, SEED = (32, 40), 8, 3, 3


# ---------------------------------------------------------------- the draw
def test_photo_draw_stays_inside_its_ranges():
    B, C, G, P = BCGP
    draws = [photo_draw(SEED, i % 7, i, i % 4, B, C, G, P) for i in range(10000)]
    b, c, g = (np.array([d[j] for d in draws]) for j in range(3))
    gray = np.array([d[3] for d in draws])
    assert b.min() >= -B and b.max() <= B and b.min() < -0.9 * B and b.max() > 0.9 * B
    assert c.min() >= 1 / (1 + C) and c.max() <= 1 + C and c.min() < 1 / (1 + 0.9 * C) and c.max() > 1 + 0.9 * C
    assert g.min() >= 1 / G and g.max() <= G and g.min() < 1 / (0.95 * G) and g.max() > 0.95 * G
    assert all(type(d[3]) is bool for d in draws[:10])
    # gray is Bernoulli(P): the frequency over n draws is within 3 sigma of P
    assert abs(gray.mean() - P) <= 3 * math.sqrt(P * (1 - P) / len(draws))
    # the centres: b is symmetric, log c and log g are symmetric
    assert abs(b.mean()) < 0.01 and abs(np.log(c).mean()) < 0.01 and abs(np.log(g).mean()) < 0.01
    # nothing to draw: the identity, never gray; certain gray
    assert all(photo_draw(SEED, 0, i, 0, 0, 0, 1, 0) == (0.0, 1.0, 1.0, False) for i in range(100))
    assert all(photo_draw(SEED, 0, i, 0, 0, 0, 1, 1)[3] for i in range(100))


def test_photo_draw_is_a_function_of_seed_epoch_index_k_only():
    B, C, G, P = BCGP
    a = [photo_draw(3, 2, 7, k, B, C, G, P) for k in range(4)]                 # as K = 4 draws them
    assert a[0] == photo_draw(3, 2, 7, 0, B, C, G, P)                          # as K = 1 draws crop 0
    assert a[::-1] == [photo_draw(3, 2, 7, k, B, C, G, P) for k in (3, 2, 1, 0)]          # any call order
    assert len({d[:3] for d in a}) == 4
    assert a[0] not in (photo_draw(4, 2, 7, 0, B, C, G, P), photo_draw(3, 3, 7, 0, B, C, G, P),
                        photo_draw(3, 2, 8, 0, B, C, G, P))
    # the documented chain: slots 5..8 of the crop's draw state
    s = DS._draw_state(5, 9, 123, 2)
    u = [(DS._splitmix64(s ^ j) >> 11) / 2 ** 53 for j in (5, 6, 7, 8)]
    assert photo_draw(5, 9, 123, 2, B, C, G, P) == (B * (2 * u[0] - 1), (1 + C) ** (2 * u[1] - 1),
                                                    G ** (2 * u[2] - 1), u[3] < P)


def test_crop_and_scale_draws_are_what_they_were():
    """Literals computed with the code before photo_draw existed."""
    args = [(0, 0, 0, 0), (3, 1, 7, 2), (12345, 17, 999, 3), (2 ** 40 + 5, 2, 0, 1)]
    assert [crop_draw(*a, 37, 101) for a in args] == [(23, 1, True), (15, 53, False), (23, 63, True), (21, 93, True)]
    assert [scale_draw(*a, 0.75, 1.33) for a in args] == [1.1669521902254036, 1.0782867021446982, 0.866523908954948,
                                                          1.0324196176403135]
    assert [scale_draw(*a, 0.25, 4.0) for a in args] == [2.124030189514557, 1.4489758089327958, 0.5029154088320726,
                                                         1.174068781309638]


# ---------------------------------------------------------------- the tone table
def test_photo_table_identity_range_and_definition():
    ident = photo_table(0, 1, 1)
    assert ident.dtype == np.float32 and ident.shape == (256,) and np.array_equal(ident, np.arange(256))
    rng = np.random.default_rng(1)
    for _ in range(200):
        b, c, g = rng.uniform(-0.5, 0.5), 2.0 ** rng.uniform(-1, 1), 2.0 ** rng.uniform(-1, 1)
        t = photo_table(b, c, g)
        assert t.dtype == np.float32 and np.isfinite(t).all() and t.min() >= 0.0 and t.max() <= 255.0
        # an independent float64 evaluation, entry by entry
        want = [255.0 * min(1.0, max(0.0, c * (math.pow(u / 255.0, g) - 0.5) + 0.5 + b)) for u in range(256)]
        assert np.abs(t.astype(np.float64) - np.array(want)).max() <= 255.0 * 2.0 ** -24 + 1e-10
        if c > 0:
            assert (np.diff(t) >= 0).all()                       # gamma and a positive contrast keep the order
    assert np.array_equal(photo_table(0.5, 1, 1)[128:], np.full(128, 255.0, dtype=np.float32))       # clipped at white
    assert np.array_equal(photo_table(-0.5, 1, 1)[:128], np.zeros(128, dtype=np.float32))            # and at black


# ---------------------------------------------------------------- apply_photo
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("gray", [False, True])
def test_apply_photo(c, gray):
    rng = np.random.default_rng(10 * c + gray)
    img = rng.integers(0, 256, (9, 13, c) if c > 1 else (9, 13), dtype=np.uint8)
    # the identity table: to_unit_float of the image, exactly (gray or not for one channel)
    ident = apply_photo(img, photo_table(0, 1, 1), False)
    assert ident.dtype == np.float64 and ident.shape == (9, 13, 3)
    assert np.array_equal(ident, gray_to_rgb(to_unit_float(img)))
    table = photo_table(0.1, 1.2, 0.8)
    got = apply_photo(img, table, gray)
    assert got.shape == (9, 13, 3) and got.min() >= 0.0 and got.max() <= 1.0
    t64 = table.astype(np.float64)
    px = img.reshape(9, 13, -1)
    for y, x in [(0, 0), (8, 12), (4, 7), (3, 0)]:
        if c == 1:
            want = [t64[px[y, x, 0]]] * 3                        # gray is ignored: the one value feeds three channels
        else:
            r, g, b = (t64[px[y, x, j]] for j in range(3))       # alpha (c == 4) is ignored
            mix = float(np.float32(0.114)) * b + (float(np.float32(0.587)) * g + float(np.float32(0.299)) * r)
            want = [mix] * 3 if gray else [r, g, b]
        assert got[y, x].tolist() == [v / 255.0 for v in want]
    if c == 1:
        assert np.array_equal(got, apply_photo(img[:, :, None], table, not gray))
    with pytest.raises(ValueError):
        apply_photo(img.astype(np.float32), table, gray)
    with pytest.raises(ValueError):
        apply_photo(img, table.astype(np.float64), gray)


# ---------------------------------------------------------------- dataset
SIZES = [(40, 56), (20, 30), (90, 150)]


@pytest.fixture(scope="module")
def tiny_root(tmp_path_factory):
    """Three PNG images of mixed size (one smaller than the crop) with maps and head sidecars."""
    from PIL import Image
    root = tmp_path_factory.mktemp("photo_ds")
    img_root, gt_root = root / "images", root / "ground_truth"
    img_root.mkdir(), gt_root.mkdir()
    rng = np.random.default_rng(11)
    for k, (h, w) in enumerate(SIZES):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(img_root / f"IMG_{k}.png")
        p = np.stack([rng.random(12 + 9 * k) * w, rng.random(12 + 9 * k) * h], 1)
        np.save(gt_root / f"IMG_{k}.npy", gaussian_filter_density((h, w), p))
        np.save(heads_path(str(gt_root / f"IMG_{k}.npy")), heads_table(p, (h, w)))
    return str(img_root), str(gt_root)


def _kw(scale, heads, **more):
    return dict(gt_downsample=D, phase="train", seed=SEED, crop=CROP, crops_per_image=K, crop_scale=scale,
                gt_from_heads=heads, **more)


@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("scale", [None, (0.5, 2.0)])
def test_dataset_items(tiny_root, scale, heads):
    img_root, gt_root = tiny_root
    B, C, G, P = BCGP
    from can_distributed_pytorch_amd.data.dataset import imread
    for raw in (False, True):
        off = CrowdDataset(img_root, gt_root, raw=raw, **_kw(scale, heads))
        zero = CrowdDataset(img_root, gt_root, raw=raw, gray_prob=0.0, **_kw(scale, heads))      # the defaults: off
        on = CrowdDataset(img_root, gt_root, raw=raw, photo_jitter=(B, C, G), gray_prob=P, **_kw(scale, heads))
        ident = CrowdDataset(img_root, gt_root, raw=raw, photo_jitter=(0, 0, 1), **_kw(scale, heads))
        for i, (h0, w0) in enumerate(SIZES):
            a, z, b, e = off[(i, 2)], zero[(i, 2)], on[(i, 2)], ident[(i, 2)]
            # off: the items of before, and everything but the colours is untouched by the feature
            assert len(a) == len(z) == (3 if raw else 2) and all(torch.equal(x, y) for x, y in zip(a, z))
            assert len(b) == len(e) == (4 if raw else 2)
            assert all(torch.equal(x, y) for x, y in zip(a[1:3], b[1:3]))
            rows = []
            for k in range(K):
                bb, cc, gg, gray = photo_draw(SEED, 2, i, k, B, C, G, P)
                rows.append(np.concatenate([photo_table(bb, cc, gg), [np.float32(gray)]]).astype(np.float32))
            if raw:
                assert torch.equal(a[0], b[0]) and torch.equal(a[0], e[0])
                assert b[3].dtype == torch.float32 and tuple(b[3].shape) == (K, 257)
                assert np.array_equal(b[3].numpy(), np.stack(rows))
                assert np.array_equal(e[3].numpy(), np.tile(np.arange(257, dtype=np.float32) % 256, (K, 1)))
                continue
            assert torch.equal(a[0], e[0])                       # the identity table changes no bit of a CPU item
            img = imread(os.path.join(img_root, f"IMG_{i}.png"))
            for k in range(K):
                if scale is None:
                    wh, ww = crop_window(h0, w0, *CROP, D)
                else:
                    wh, ww = scaled_window(h0, w0, *CROP, scale_draw(SEED, 2, i, k, *scale))
                y0, x0, fl = crop_draw(SEED, 2, i, k, h0 - wh + 1, w0 - ww + 1)
                win = apply_photo(_as_uint8(img[y0:y0 + wh, x0:x0 + ww]), rows[k][:256], bool(rows[k][256]))
                dm = np.zeros((wh, ww), dtype=np.float32)
                want = prepare_pair_scaled(win, dm, *CROP, D, fl)[0] if scale else prepare_pair(win, dm, D, fl)[0]
                got = b[0][k].numpy()
                assert np.array_equal(got[:, :want.shape[1], :want.shape[2]], want)
                assert not got[:, want.shape[1]:].any() and not got[:, :, want.shape[2]:].any()      # padding stays 0
            assert not torch.equal(a[0], b[0])


def test_dataset_argument_errors_and_eval_phase(tiny_root):
    img_root, gt_root = tiny_root
    with pytest.raises(ValueError, match="crop"):
        CrowdDataset(img_root, gt_root, gt_downsample=D, photo_jitter=(0.2, 0.3, 1.5))
    with pytest.raises(ValueError, match="crop"):
        CrowdDataset(img_root, gt_root, gt_downsample=D, gray_prob=0.3)
    for bad in ((-0.1, 0, 1), (0.6, 0, 1), (0, -0.1, 1), (0, 1.1, 1), (0, 0, 0.9), (0, 0, 2.1), (float("nan"), 0, 1),
                (0.1, 0.2)):
        with pytest.raises(ValueError):
            CrowdDataset(img_root, gt_root, gt_downsample=D, crop=CROP, photo_jitter=bad)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            CrowdDataset(img_root, gt_root, gt_downsample=D, crop=CROP, gray_prob=bad)
    # evaluation is untouched: the whole-image items of a test-phase dataset without the options
    plain = CrowdDataset(img_root, gt_root, gt_downsample=D, phase="test", raw=True)
    ev = CrowdDataset(img_root, gt_root, gt_downsample=D, phase="test", raw=True, crop=CROP,
                      photo_jitter=(0.2, 0.3, 1.5), gray_prob=1.0)
    a, b = plain[0], ev[0]
    assert len(a) == len(b) == 3 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


# ---------------------------------------------------------------- collate
@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("scale", [None, (0.5, 2.0)])
def test_collate_appends_the_photo_region(tiny_root, scale, heads):
    img_root, gt_root = tiny_root
    B, C, G, P = BCGP
    off = CrowdDataset(img_root, gt_root, raw=True, **_kw(scale, heads))
    on = CrowdDataset(img_root, gt_root, raw=True, photo_jitter=(B, C, G), gray_prob=P, **_kw(scale, heads))
    items_off, items_on = [off[(i, 1)] for i in range(3)], [on[(i, 1)] for i in range(3)]
    ckw = dict(crop=CROP, crop_scale=scale is not None, gt_from_heads=heads)
    b_off, m_off = PackedCollate(**ckw)(items_off)
    buf, meta = PackedCollate(photo=True, **ckw)(items_on)
    n, goff, doff = m_off[0], m_off[3], m_off[4]
    ioff = sum(h * w * 3 for h, w in SIZES)                      # (the alignment gap behind the images is not written)
    # nine fields: (n, Ho, Wo, gt_offset, desc_offset, images, kind, heads, photo_offset)
    assert len(meta) == 9 and meta[:5] == m_off[:5] and n == 3 * K
    assert meta[5:8] == (3, 2 if scale else 1, m_off[7] if heads else -1)
    poff = meta[8]
    assert poff == b_off.numel() and poff % 16 == 0 and buf.numel() == poff + 4 * 260 * n
    # the images, ground truth, descriptors, ranges and head table: the pack without the feature, byte for byte
    assert torch.equal(buf[:ioff], b_off[:ioff]) and torch.equal(buf[goff:poff], b_off[goff:])
    region = buf[poff:].view(torch.float32).view(n, 260)
    assert torch.equal(region[:, :257], torch.cat([it[3] for it in items_on])) and not region[:, 257:].any()
    kind = ("crop_scaled" if scale else "crop") + ("+heads" if heads else "")
    _, dims, got_kind = _unpack((buf, meta))
    assert dims == m_off[:5] and got_kind == kind + "+photo" and _unpack((b_off, m_off))[2] == kind
    # mismatched items, either way
    with pytest.raises(ValueError, match="photo"):
        PackedCollate(photo=True, **ckw)(items_off)
    with pytest.raises(ValueError, match="photo"):
        PackedCollate(**ckw)(items_on)
    with pytest.raises(ValueError, match="photo"):
        PackedCollate(photo=True, **ckw)([it[:3] + (it[3][:, :256],) for it in items_on])
    with pytest.raises(ValueError, match="photo"):
        PackedCollate(photo=True, **ckw)([it[:3] + (it[3][:-1],) for it in items_on])
    # a truncated buffer, a buffer with bytes to spare, a misplaced or misaligned region, a bad kind
    for bad in ((buf[:-16], meta), (buf[:-4 * 260], meta), (torch.cat([buf, buf[:16]]), meta),
                (buf, meta[:8] + (poff + 16,)), (buf[:-8], meta[:8] + (poff - 8,)), (buf, meta[:6] + (0,) + meta[7:]),
                (buf, meta[:6] + (3,) + meta[7:]), (buf, meta[:7] + (-2, poff))):
        with pytest.raises(ValueError, match="packed batch"):
            _unpack(bad)


def test_collate_photo_needs_crop():
    with pytest.raises(ValueError, match="crop"):
        PackedCollate(photo=True)


# ---------------------------------------------------------------- train.py
def test_train_py_photo_options():
    sys.path.insert(0, ROOT)
    try:
        import train
    finally:
        sys.path.remove(ROOT)
    p = train.build_parser()
    a = p.parse_args([])
    assert a.photo_jitter is None and a.gray_prob is None
    a = p.parse_args(["--crop-size", "64x96", "--photo-jitter", "0.2,0.3,1.5", "--gray-prob", "0.3"])
    assert a.photo_jitter == (0.2, 0.3, 1.5) and a.gray_prob == 0.3
    assert p.parse_args(["--crop-size", "64x96", "--photo-jitter", "0,0,1"]).photo_jitter == (0.0, 0.0, 1.0)
    assert p.parse_args(["--crop-size", "64x96", "--photo-jitter", "0.5,1,2"]).photo_jitter == (0.5, 1.0, 2.0)
    assert p.parse_args(["--crop-size", "64x96", "--gray-prob", "1"]).gray_prob == 1.0
    crop = ["--crop-size", "64x96"]
    for bad in (["--photo-jitter", "0.2,0.3,1.5"], ["--gray-prob", "0.3"],                       # without --crop-size
                ["--synthetic", "64x96", "--photo-jitter", "0.2,0.3,1.5"], ["--synthetic", "64x96", "--gray-prob", "0.3"],
                crop + ["--photo-jitter", "0.2,0.3"], crop + ["--photo-jitter", "0.2,0.3,1.5,1"],
                crop + ["--photo-jitter", "a,b,c"], crop + ["--photo-jitter", "-0.1,0,1"],
                crop + ["--photo-jitter", "0.6,0,1"], crop + ["--photo-jitter", "0,-0.1,1"],
                crop + ["--photo-jitter", "0,1.1,1"], crop + ["--photo-jitter", "0,0,0.9"],
                crop + ["--photo-jitter", "0,0,2.1"], crop + ["--photo-jitter", "nan,0,1"],
                crop + ["--gray-prob", "-0.1"], crop + ["--gray-prob", "1.1"], crop + ["--gray-prob", "nan"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
