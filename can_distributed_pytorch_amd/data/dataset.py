"""CrowdDataset — reference data contract (model/CrowdDataset.py:11-69).

``CrowdDataset(img_root, gt_dmap_root, gt_downsample=1, phase='train')``
lists the files of ``img_root``; item i = (image [3,H',W'] float32 ImageNet-
normalised, density [1,H'/d,W'/d] float32) with H', W' the largest multiples
of d, a random horizontal flip of BOTH in phase 'train', and the ground
truth loaded from ``gt_dmap_root/<name>.npy`` (``.jpg`` -> ``.npy``).

Differences: gt_downsample <= 1 works (Q8), integer
images only are /255 (Q14), decoding uses PIL (cv2 is not a dependency).
The random flip (model/CrowdDataset.py:48-50, Python ``random`` there) is a
pure function of (seed, epoch, index) — a counter-based hash, no RNG state:
DataLoader workers cannot replay one another's stream (a ``random.Random``
pickled into every worker would), and a resumed run draws exactly the flips
of an uninterrupted one.  The epoch comes from ``set_epoch`` or, with
worker processes, travels with the index (``EpochTaggedSampler``).
``crop=(ch, cw)`` (train phase only) turns an item into ``crops_per_image``
random windows of that size of the one decoded image, each with its own
offset and flip drawn by ``crop_draw`` from (seed, epoch, index, k), zero-padded
where the image is smaller than the crop (README, "Random-crop training").
``crop_scale=(lo, hi)`` adds a random scale per crop (``scale_draw``): a window of
(ch, cw) / s is resampled to the crop, never padded (README, "Random-scale crops").
``gt_from_heads=True`` (with ``crop``) renders every crop's ground truth from the image's head records
(``IMG_k.heads.npy``, data/density.py:heads_table) as exact area sums instead of resampling the density map, which
is then never opened (README, "Ground truth from heads").
``photo_jitter=(B, C, G)`` / ``gray_prob=P`` (with ``crop``) jitter every crop's colours: brightness, contrast and gamma as
one 256-entry tone table per crop (``photo_draw``, ``transforms.photo_table``) applied to the source bytes before the
flip and the resample, and a random luma mix (README, "Photometric jitter").
``SyntheticCrowdDataset`` provides the same item contract without files
(benchmarks, tests, smoke runs).
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch
from torch.utils.data import Dataset

from .transforms import (_axis_weights, apply_photo, area_factor, heads_to_gt, heads_to_gt_padded, photo_table,
                         prepare_pair, prepare_pair_scaled, roi_weights, roi_weights_padded)

IMG_EXT = (".jpg", ".jpeg", ".png", ".bmp", ".tif", ".tiff")
_M64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def flip_draw(seed: int, epoch: int, index: int) -> bool:
    """The p=0.5 horizontal flip of sample ``index`` in ``epoch`` (stateless, worker-independent)."""
    return bool(_splitmix64(_splitmix64(_splitmix64(seed & _M64) ^ (epoch & _M64)) ^ (index & _M64)) >> 63)


def crop_window(h0: int, w0: int, ch: int, cw: int, downsample: int = 8):
    """(vh, vw): the extent of a (ch, cw) crop inside an h0 x w0 image -- the crop itself, or the image's largest
    multiple of the downsample where the image is smaller (the rest of the crop is zero padding)."""
    return min(ch, h0 // downsample * downsample), min(cw, w0 // downsample * downsample)


def _draw_state(seed: int, epoch: int, index: int, k: int) -> int:
    """The splitmix64 chain over (seed, epoch, index, k) that the draws of crop ``k`` hash once more per value."""
    return _splitmix64(_splitmix64(_splitmix64(_splitmix64(seed & _M64) ^ (epoch & _M64)) ^ (index & _M64)) ^ (k & _M64))


def crop_draw(seed: int, epoch: int, index: int, k: int, ny: int, nx: int):
    """Crop ``k`` of sample ``index`` in ``epoch``: (y0 uniform on [0, ny), x0 uniform on [0, nx), p=0.5 flip).
    Stateless like ``flip_draw`` (one splitmix64 chain over seed, epoch, index, k, then one hash per drawn value),
    so it depends neither on a worker's history nor on how many crops an image yields."""
    s = _draw_state(seed, epoch, index, k)
    y0 = (_splitmix64(s ^ 1) * max(1, int(ny))) >> 64          # multiply-shift: bias < n / 2^64
    x0 = (_splitmix64(s ^ 2) * max(1, int(nx))) >> 64
    return int(y0), int(x0), bool(_splitmix64(s ^ 3) >> 63)


def scale_draw(seed: int, epoch: int, index: int, k: int, lo: float, hi: float) -> float:
    """The scale of crop ``k`` of sample ``index`` in ``epoch``: log-uniform on [lo, hi], > 1 magnifies.  One more hash
    of ``crop_draw``'s chain state, so it is as stateless (no dependence on K, workers or resumes) and leaves the
    offset and flip draws what they are."""
    s = _draw_state(seed, epoch, index, k)
    u = (_splitmix64(s ^ 4) >> 11) / 2 ** 53
    return float(min(hi, max(lo, lo * (hi / lo) ** u)))


def check_crop_scale(lo, hi):
    """(lo, hi) as floats, or ValueError: 0.25 <= lo <= hi <= 4 (the range the scaled crop kernel accepts)."""
    lo, hi = float(lo), float(hi)
    if not (0.0 < lo <= hi) or lo < 0.25 or hi > 4.0:
        raise ValueError(f"crop scale range must satisfy 0.25 <= lo <= hi <= 4, got {lo},{hi}")
    return lo, hi


def photo_draw(seed: int, epoch: int, index: int, k: int, B: float, C: float, G: float, P: float):
    """The photometric jitter of crop ``k`` of sample ``index`` in ``epoch``: (b, c, g, gray) with the brightness shift b
    uniform on [-B, B], the contrast factor c log-uniform on [1/(1+C), 1+C], the gamma g log-uniform on [1/G, G] and
    gray with probability P.  Four more hashes of ``crop_draw``'s chain state (slots 5..8; 1..3 are crop_draw's, 4 is
    scale_draw's), so it is as stateless and leaves the other draws what they are."""
    s = _draw_state(seed, epoch, index, k)
    u5, u6, u7, u8 = ((_splitmix64(s ^ j) >> 11) / 2 ** 53 for j in (5, 6, 7, 8))
    return float(B * (2 * u5 - 1)), float((1.0 + C) ** (2 * u6 - 1)), float(G ** (2 * u7 - 1)), bool(u8 < P)


def check_photo(photo_jitter, gray_prob):
    """((B, C, G), P) as floats, or ValueError: 0 <= B <= 0.5, 0 <= C <= 1, 1 <= G <= 2, 0 <= P <= 1.  No jitter is
    (0, 0, 1), the identity table."""
    try:
        B, C, G = (float(v) for v in ((0.0, 0.0, 1.0) if photo_jitter is None else photo_jitter))
    except (TypeError, ValueError):
        raise ValueError(f"photo jitter is (B, C, G), got {photo_jitter!r}")
    P = float(gray_prob)
    if not (0.0 <= B <= 0.5 and 0.0 <= C <= 1.0 and 1.0 <= G <= 2.0):
        raise ValueError(f"photo jitter must satisfy 0 <= B <= 0.5, 0 <= C <= 1, 1 <= G <= 2, got {B},{C},{G}")
    if not 0.0 <= P <= 1.0:
        raise ValueError(f"gray probability must be in [0, 1], got {P}")
    return (B, C, G), P


def scaled_window(h0: int, w0: int, ch: int, cw: int, s: float):
    """(sh, sw): the source extent that scale ``s`` resamples to a (ch, cw) crop of an h0 x w0 image.  The scale is
    raised to what makes the window fit (s_eff = max(s, ch/h0, cw/w0)): the crop is always fully valid, and an image
    smaller than the crop is upsampled to fill it (the unscaled path pads it instead).  float64 on the host; the
    kernel sees the integers only."""
    s_eff = max(float(s), ch / h0, cw / w0)
    sh = min(h0, max(1, int(np.floor(ch / s_eff + 0.5))))
    sw = min(w0, max(1, int(np.floor(cw / s_eff + 0.5))))
    return sh, sw


def _as_uint8(img: np.ndarray) -> np.ndarray:
    """The decoded image as the writable, C-contiguous uint8 array the GPU path packs: float images are x255, every
    other type is clipped to [0, 255]."""
    if img.dtype != np.uint8:
        img = np.clip(np.asarray(img, dtype=np.float64) * (255.0 if img.dtype.kind == "f" else 1.0),
                      0, 255).astype(np.uint8)
    return np.require(img, requirements=("C", "W"))


def _pad_to(a: np.ndarray, h: int, w: int) -> np.ndarray:
    """Zero-pad the last two axes at the bottom / right to (h, w)."""
    if a.shape[-2:] == (h, w):
        return a
    out = np.zeros(a.shape[:-2] + (h, w), dtype=a.dtype)
    out[..., :a.shape[-2], :a.shape[-1]] = a
    return out


def crop_collate(batch):
    """collate_fn for CrowdDataset(crop=..., raw=False): the K-stacks of a batch, concatenated to [B*K, ...]."""
    imgs, gts = zip(*batch)
    return torch.cat(imgs), torch.cat(gts)


def _density_resize(dmap: np.ndarray, rows: int, cols: int, flip: bool) -> np.ndarray:
    """Optional flip, then the cv2 INTER_LINEAR resize of a 2-D density map of any size to (rows, cols), float64."""
    if dmap.ndim != 2:
        raise ValueError(f"density must be a 2-D map, got shape {tuple(dmap.shape)}")
    hd, wd = (int(v) for v in dmap.shape)
    if (rows, cols) == (hd, wd):
        return np.asarray(dmap, dtype=np.float64)[:, ::-1] if flip else np.asarray(dmap, dtype=np.float64)
    # gather the rows the vertical taps use first (a memory-mapped map is read only there), then resize
    y0, y1, fy = _axis_weights(hd, rows)
    x0, x1, fx = _axis_weights(wd, cols)
    if flip:                                 # flip before resize == mirrored column taps
        x0, x1 = wd - 1 - x0, wd - 1 - x1
    need = np.unique(np.concatenate([y0, y1]))
    sub = np.asarray(dmap[need], dtype=np.float64)
    pos = np.searchsorted(need, np.arange(hd))
    r = sub[pos[y0]] * (1.0 - fy)[:, None] + sub[pos[y1]] * fy[:, None]
    return r[:, x0] * (1.0 - fx)[None] + r[:, x1] * fx[None]


def density_to_gt(dmap: np.ndarray, h: int, w: int, downsample: int, flip: bool) -> np.ndarray:
    """The density half of prepare_pair (model/CrowdDataset.py:48-62): optional flip, cv2 INTER_LINEAR resize of a
    density map of ANY size to (W//d, H//d) of the IMAGE's size (reference :60 resizes whatever map it loaded), x d^2.
    Returns fp32 [1, H//d, W//d]."""
    dm = _density_resize(dmap, h // downsample, w // downsample, flip)
    return (dm * (downsample * downsample))[None].astype(np.float32)


def density_to_gt_scaled(dmap: np.ndarray, ch: int, cw: int, downsample: int, flip: bool) -> np.ndarray:
    """The density half of prepare_pair_scaled: a density WINDOW of any extent (sh, sw) -> the ground truth of the
    (ch, cw) sample it is resampled to, x (sh*sw) / cells (the area ratio, d^2 for an unscaled window).  Row-gathered
    like density_to_gt.  Returns fp32 [1, ch//d, cw//d]."""
    rows, cols = ch // downsample, cw // downsample
    dm = _density_resize(dmap, rows, cols, flip).astype(np.float32)
    return (dm * area_factor(dmap.shape[0], dmap.shape[1], rows, cols))[None]


class EpochTaggedSampler:
    """Wraps a sampler (e.g. DistributedSampler) so that every index carries the sampler's epoch:
    yields (index, epoch) pairs, which ``CrowdDataset.__getitem__`` accepts.  Needed because persistent
    DataLoader workers hold their own copy of the dataset (``dataset.set_epoch`` in the main process would
    not reach them)."""

    def __init__(self, sampler):
        self.sampler = sampler

    def set_epoch(self, epoch: int):
        self.sampler.set_epoch(epoch)

    def __iter__(self):
        ep = int(getattr(self.sampler, "epoch", 0))
        for i in self.sampler:
            yield (int(i), ep)

    def __len__(self):
        return len(self.sampler)

    def __getattr__(self, name):          # total_size, num_replicas, ... of the wrapped sampler
        return getattr(self.sampler, name)


def imread(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB", "RGBA"):
            im = im.convert("RGB")
        return np.asarray(im)


class CrowdDataset(Dataset):
    def __init__(self, img_root: str, gt_dmap_root: str, gt_downsample: int = 1, phase: str = "train",
                 seed: Optional[int] = None, raw: bool = False, crop=None, crops_per_image: int = 1,
                 crop_scale=None, gt_from_heads: bool = False, photo_jitter=None, gray_prob: float = 0.0,
                 roi: bool = False):
        self.img_root = img_root
        # roi=True: every image has an ROI mask ground_truth/NAME.roi.npy (data/density.py:roi_path).  raw=False items
        # carry a 2-channel ground truth (the ground truth, the per-cell loss weight of transforms.roi_weights);
        # raw=True items carry the image as uint8 [H0, W0, 4] with the mask as its alpha channel and the GPU renders
        # the weights (ops/preprocess.py roi=True).  Every phase and kind alike.
        self.roi = bool(roi)
        self.gt_dmap_root = gt_dmap_root
        self.gt_downsample = max(1, int(gt_downsample))
        self.phase = phase
        self.img_names = sorted(f for f in os.listdir(img_root)
                                if os.path.isfile(os.path.join(img_root, f)) and f.lower().endswith(IMG_EXT))
        self.n_samples = len(self.img_names)
        self.seed = 0 if seed is None else int(seed)
        self.epoch = 0
        # raw=True: return (uint8 image, full-res density, flip) and let the GPU
        # preprocess it (ops/preprocess.py) instead of resizing on the CPU
        self.raw = raw
        # crop=(ch, cw): a train item is crops_per_image random windows of that size of ONE decoded image (each with
        # its own offset and flip, crop_draw), zero-padded where the image is smaller; test items stay whole images
        self.crop = None
        self.crops_per_image = int(crops_per_image)
        if crop is not None and phase == "train":
            ch, cw = (int(v) for v in crop)
            if ch <= 0 or cw <= 0 or ch % self.gt_downsample or cw % self.gt_downsample:
                raise ValueError(f"crop {ch}x{cw} must be a positive multiple of the downsample {self.gt_downsample}")
            if self.crops_per_image < 1:
                raise ValueError(f"crops_per_image must be >= 1, got {crops_per_image}")
            self.crop = (ch, cw)
        # crop_scale=(lo, hi): every crop resamples a window of (ch, cw) / s, s log-uniform on [lo, hi] (scale_draw)
        self.crop_scale = None
        if crop_scale is not None:
            if crop is None:
                raise ValueError("crop_scale needs crop=(ch, cw)")
            lo_hi = check_crop_scale(*crop_scale)
            if self.crop is not None:
                self.crop_scale = lo_hi
        # gt_from_heads: the crops' ground truth is rendered from the head sidecars (exact area sums), no map is opened
        if gt_from_heads and crop is None:
            raise ValueError("gt_from_heads needs crop=(ch, cw): it renders the ground truth of crop windows")
        self.gt_from_heads = bool(gt_from_heads) and self.crop is not None
        # photo_jitter=(B, C, G) / gray_prob=P: every crop's source bytes go through its own tone table and, with
        # probability P, the luma mix (photo_draw); either one switches it on
        self.photo = None
        if photo_jitter is not None or gray_prob:
            if crop is None:
                raise ValueError("photo_jitter / gray_prob need crop=(ch, cw): they jitter the crops' colours")
            bcg, p = check_photo(photo_jitter, gray_prob)
            if self.crop is not None:
                self.photo = bcg + (p,)

    def __len__(self):
        return self.n_samples

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def gt_path(self, name: str) -> str:
        stem = os.path.splitext(name)[0]
        return os.path.join(self.gt_dmap_root, stem + ".npy")

    def load_heads(self, name: str) -> np.ndarray:
        """The head records float32 [N, 4] of image ``name`` from its sidecar next to the density map."""
        from .density import heads_path
        path = heads_path(self.gt_path(name))
        if not os.path.isfile(path):
            raise ValueError(f"{name}: no head sidecar {path}; write the sidecars with "
                             "`python data_preparation/k_nearest_gaussian_kernel.py <dataset root> --heads`")
        heads = np.load(path)                                    # allow_pickle=False (default)
        if heads.ndim != 2 or heads.shape[1] != 4:
            raise ValueError(f"{path}: head records must be [N, 4] of (c, r, sigma, R), got {tuple(heads.shape)}")
        return np.ascontiguousarray(heads, dtype=np.float32)

    def load_roi(self, name: str, h0: int, w0: int) -> np.ndarray:
        """The ROI mask uint8 [h0, w0] of image ``name``; a missing or mis-shaped one is a ValueError naming the file."""
        from .density import roi_path
        path = roi_path(self.gt_path(name))
        if not os.path.isfile(path):
            raise ValueError(f"{name}: no ROI mask {path} (uint8 [H0, W0], 255 inside the region of interest)")
        mask = np.load(path)                                     # allow_pickle=False (default)
        if mask.dtype != np.uint8 or tuple(mask.shape) != (h0, w0):
            raise ValueError(f"{path}: an ROI mask is uint8 {(h0, w0)} like its image, got {mask.dtype} "
                             f"{tuple(mask.shape)}")
        return np.ascontiguousarray(mask)

    @staticmethod
    def _with_alpha(img: np.ndarray, mask: np.ndarray) -> np.ndarray:
        """uint8 [H0, W0, 4]: the image's three colour channels (a gray image's value three times) and the mask as
        alpha; an alpha channel of the image's own is replaced."""
        img = _as_uint8(img)
        rgb = np.repeat(img[:, :, None], 3, axis=2) if img.ndim == 2 else img[:, :, :3]
        if rgb.shape[2] != 3:
            raise ValueError(f"an image is L, RGB or RGBA, got {tuple(img.shape)}")
        return np.ascontiguousarray(np.concatenate([rgb, mask[:, :, None]], axis=2))

    def __getitem__(self, index):
        epoch = self.epoch
        if isinstance(index, (tuple, list)):
            index, epoch = int(index[0]), int(index[1])
        if not 0 <= index < len(self):
            raise IndexError("index range error")
        name = self.img_names[index]
        img = imread(os.path.join(self.img_root, name))
        if self.crop is not None:
            return self._crop_item(img, name, epoch, index)
        flip = self.phase == "train" and flip_draw(self.seed, epoch, index)
        d = self.gt_downsample
        mask = self.load_roi(name, img.shape[0], img.shape[1]) if self.roi else None
        if self.raw:
            # the GPU resizes / normalises the image; the ground truth is brought to its 1/d resolution here,
            # reading only the source rows the bilinear taps touch (memory-mapped: ~1/4 of a full-resolution
            # fp32 map), so a batch moves ~8x fewer host bytes than shipping full-resolution densities
            dmap = np.load(self.gt_path(name), mmap_mode="r")        # allow_pickle=False (default)
            gt = density_to_gt(dmap, img.shape[0], img.shape[1], self.gt_downsample, flip)
            img = _as_uint8(img) if mask is None else self._with_alpha(img, mask)
            return torch.from_numpy(img), torch.from_numpy(gt), flip
        dmap = np.load(self.gt_path(name))                       # allow_pickle=False (default)
        im, dm = prepare_pair(img, dmap, self.gt_downsample, flip)
        if mask is not None:
            h0, w0 = mask.shape
            dm = np.concatenate([dm, roi_weights(mask, 0, 0, h0, w0, h0 // d, w0 // d, flip)[None]])
        return torch.from_numpy(np.ascontiguousarray(im)), torch.from_numpy(np.ascontiguousarray(dm))


    def _crop_item(self, img: np.ndarray, name: str, epoch: int, index: int):
        """K crops of one decoded image, crop k the window (y0, x0, wh, ww) placed by crop_draw: the (vh, vw) of
        crop_window, zero-padded to the crop, or with crop_scale the scaled_window of its scale_draw, resampled to it.
        raw=False: ([K,3,ch,cw] f32, [K,1,ch/d,cw/d] f32), each prepare_pair / prepare_pair_scaled of the window's
        slices.  raw=True: (uint8 image, [K,1,ch/d,cw/d] f32, int64 windows [K,3] of (y0, x0, flip) or, scaled, [K,5]
        of (y0, x0, flip, sh, sw)): the GPU cuts the windows (ops/preprocess.py), the ground truths are made here from
        the memory-mapped map.  gt_from_heads: the same windows; raw=False renders each ground truth with heads_to_gt /
        heads_to_gt_padded, raw=True returns the image's head records [N, 4] in place of the K ground truths (the GPU
        renders them); no density map is opened.  With photo_jitter / gray_prob: raw=False takes apply_photo of the
        window's bytes (a float image, which prepare_pair[_scaled] keep) in place of the window; raw=True items gain a
        fourth element, _photo_rows' float32 [K, 257], and the GPU applies the tables."""
        d, (ch, cw), K = self.gt_downsample, self.crop, self.crops_per_image
        h0, w0 = img.shape[:2]
        scaled = self.crop_scale is not None
        if self.gt_from_heads:
            return self._crop_item_heads(img, self.load_heads(name), epoch, index, scaled, name)
        dmap = np.load(self.gt_path(name), mmap_mode="r" if self.raw else None)      # allow_pickle=False (default)
        if tuple(dmap.shape) != (h0, w0):
            raise ValueError(f"{name}: density map {tuple(dmap.shape)} differs from its image {(h0, w0)}: a crop "
                             "takes the same window of both")
        ims, gts, rows = [], [], []
        photo = self._photo_rows(epoch, index)
        mask = self.load_roi(name, h0, w0) if self.roi else None
        for k in range(K):
            if scaled:
                wh, ww = scaled_window(h0, w0, ch, cw, scale_draw(self.seed, epoch, index, k, *self.crop_scale))
            else:
                wh, ww = crop_window(h0, w0, ch, cw, d)
            y0, x0, fl = crop_draw(self.seed, epoch, index, k, h0 - wh + 1, w0 - ww + 1)
            im, dm = img[y0:y0 + wh, x0:x0 + ww], dmap[y0:y0 + wh, x0:x0 + ww]
            rows.append([y0, x0, int(fl)] + ([wh, ww] if scaled else []))
            if photo is not None and not self.raw:
                im = apply_photo(_as_uint8(im), photo[k, :256], bool(photo[k, 256]))
            if self.raw:
                gt = density_to_gt_scaled(dm, ch, cw, d, fl) if scaled else density_to_gt(dm, wh, ww, d, fl)
            else:
                im, gt = prepare_pair_scaled(im, dm, ch, cw, d, fl) if scaled else prepare_pair(im, dm, d, fl)
                ims.append(_pad_to(im, ch, cw))
            gts.append(_pad_to(gt, ch // d, cw // d))
            if mask is not None and not self.raw:
                gts[-1] = np.concatenate([gts[-1], self._crop_weights(mask, y0, x0, wh, ww, fl, scaled)[None]])
        gts = torch.from_numpy(np.stack(gts))
        if self.raw:
            img = _as_uint8(img) if mask is None else self._with_alpha(img, mask)
            return (torch.from_numpy(img), gts, torch.tensor(rows, dtype=torch.int64)) + \
                (() if photo is None else (torch.from_numpy(photo),))
        return torch.from_numpy(np.stack(ims)), gts

    def _crop_weights(self, mask: np.ndarray, y0: int, x0: int, wh: int, ww: int, fl: bool, scaled: bool):
        """The loss weights fp32 [ch/d, cw/d] of one crop window: roi_weights of a scaled window, roi_weights_padded
        (0 in the padding cells) of an unscaled one."""
        d, (ch, cw) = self.gt_downsample, self.crop
        if scaled:
            return roi_weights(mask, y0, x0, wh, ww, ch // d, cw // d, fl)
        return roi_weights_padded(mask, y0, x0, ch, cw, d, fl)

    def _photo_rows(self, epoch: int, index: int):
        """float32 [K, 257], crop k's tone table (photo_table of its photo_draw) and gray flag 0.0 / 1.0; None with the
        feature off."""
        if self.photo is None:
            return None
        out = np.empty((self.crops_per_image, 257), dtype=np.float32)
        for k in range(self.crops_per_image):
            b, c, g, gray = photo_draw(self.seed, epoch, index, k, *self.photo)
            out[k, :256] = photo_table(b, c, g)
            out[k, 256] = float(gray)
        return out

    def _crop_item_heads(self, img: np.ndarray, heads: np.ndarray, epoch: int, index: int, scaled: bool, name=None):
        """_crop_item with the ground truth from head records: the windows and flips are the same draws."""
        d, (ch, cw), K = self.gt_downsample, self.crop, self.crops_per_image
        h0, w0 = img.shape[:2]
        ims, gts, rows = [], [], []
        photo = self._photo_rows(epoch, index)
        mask = self.load_roi(name, h0, w0) if self.roi else None
        for k in range(K):
            if scaled:
                wh, ww = scaled_window(h0, w0, ch, cw, scale_draw(self.seed, epoch, index, k, *self.crop_scale))
            else:
                wh, ww = crop_window(h0, w0, ch, cw, d)
            y0, x0, fl = crop_draw(self.seed, epoch, index, k, h0 - wh + 1, w0 - ww + 1)
            rows.append([y0, x0, int(fl)] + ([wh, ww] if scaled else []))
            if self.raw:
                continue
            im, zero = img[y0:y0 + wh, x0:x0 + ww], np.zeros((wh, ww), dtype=np.float32)
            if photo is not None:
                im = apply_photo(_as_uint8(im), photo[k, :256], bool(photo[k, 256]))
            im, _ = prepare_pair_scaled(im, zero, ch, cw, d, fl) if scaled else prepare_pair(im, zero, d, fl)
            ims.append(_pad_to(im, ch, cw))
            gts.append(heads_to_gt(heads, h0, w0, (y0, x0, wh, ww), ch, cw, d, fl) if scaled else
                       heads_to_gt_padded(heads, h0, w0, y0, x0, ch, cw, d, fl))
            if mask is not None:
                gts[-1] = np.concatenate([gts[-1], self._crop_weights(mask, y0, x0, wh, ww, fl, scaled)[None]])
        if self.raw:
            img = _as_uint8(img) if mask is None else self._with_alpha(img, mask)
            return (torch.from_numpy(img), torch.from_numpy(heads), torch.tensor(rows, dtype=torch.int64)) + \
                (() if photo is None else (torch.from_numpy(photo),))
        return torch.from_numpy(np.stack(ims)), torch.from_numpy(np.stack(gts))


class SyntheticCrowdDataset(Dataset):
    """Deterministic synthetic crowd images of a fixed size (same item contract)."""

    def __init__(self, n: int, height: int = 768, width: int = 1024, gt_downsample: int = 8, seed: int = 0,
                 heads=(100, 1500)):
        from .synthetic import make_synthetic_batch
        self._make = make_synthetic_batch
        self.n, self.h, self.w = n, height, width
        self.seed = seed
        self.heads = heads
        self.gt_downsample = gt_downsample
        if gt_downsample != 8:
            raise ValueError("synthetic density maps are produced at 1/8 resolution")

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        if isinstance(index, (tuple, list)):
            index = int(index[0])
        img, gt = self._make(1, self.h, self.w, seed=self.seed * 100003 + index, heads=self.heads)
        return img[0], gt[0]
