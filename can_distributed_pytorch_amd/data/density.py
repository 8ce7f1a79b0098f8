"""Geometry-adaptive Gaussian ground-truth density maps.

Reference: data_preparation/k_nearest_gaussian_kernel.py:14-92.

* ``gaussian_filter_density(img_or_shape, points)`` — CPU version with the
  reference semantics (KD-tree 4-NN, sigma = 0.1*(d1+d2+d3), single head:
  avg(shape)/4, heads at (row=int(y), col=int(x)), out-of-image heads
  skipped).  Instead of filtering a full H*W delta image per head
  (O(N*H*W)), each head adds the clipped outer product of two normalised 1-D
  Gaussians of radius int(4*sigma+0.5) — identical to
  scipy.ndimage.gaussian_filter(delta, sigma, mode='constant') (truncate 4).
* ``density_map_gpu(points, H, W)`` — the same on the GPU (csrc/density.hip:
  brute-force kNN + per-head splat).
* ``heads_table(points, shape)`` — the head records (c, r, sigma, R) the map is a sum over; ``--heads`` writes them
  as ``IMG_*.heads.npy`` sidecars, from which ``--gt-from-heads`` renders crop ground truth as exact area sums.
* ``generate_dataset_density(root)`` — the offline driver (ShanghaiTech layout:
  images/*.jpg + ground_truth/GT_IMG_*.mat -> ground_truth/IMG_*.npy).
"""
from __future__ import annotations

import glob
import os
from typing import Sequence, Tuple, Union

import numpy as np
import torch


def _shape_of(img_or_shape) -> Tuple[int, int]:
    if isinstance(img_or_shape, (tuple, list)):
        return int(img_or_shape[0]), int(img_or_shape[1])
    return int(img_or_shape.shape[0]), int(img_or_shape.shape[1])


def _kernel1d(sigma: float) -> np.ndarray:
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-0.5 * (x / sigma) ** 2)
    return k / k.sum()


def knn_sigmas(points: np.ndarray, shape: Tuple[int, int]) -> np.ndarray:
    n = len(points)
    if n == 0:
        return np.zeros(0)
    if n == 1:
        return np.array([np.average(np.array(shape, dtype=np.float64)) / 2.0 / 2.0])
    from scipy.spatial import KDTree
    tree = KDTree(points.copy(), leafsize=2048)
    k = min(4, n)
    dist, _ = tree.query(points, k=k)
    return 0.1 * dist[:, 1:].sum(axis=1)


def gaussian_filter_density(img_or_shape, points: Union[np.ndarray, Sequence]) -> np.ndarray:
    """points: [[col, row], ...] (x, y).  Returns float32 [H, W]."""
    h, w = _shape_of(img_or_shape)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    density = np.zeros((h, w), dtype=np.float64)
    if len(pts) == 0:
        return density.astype(np.float32)
    sig = knn_sigmas(pts, (h, w))
    for (x, y), s in zip(pts, sig):
        if x < 0 or y < 0:
            continue
        c, r = int(x), int(y)
        if r >= h or c >= w:
            continue
        if s <= 0:
            density[r, c] += 1.0
            continue
        k = _kernel1d(float(s))
        R = (len(k) - 1) // 2
        r0, r1 = max(0, r - R), min(h - 1, r + R)
        c0, c1 = max(0, c - R), min(w - 1, c + R)
        density[r0:r1 + 1, c0:c1 + 1] += np.outer(k[r0 - r + R:r1 - r + R + 1], k[c0 - c + R:c1 - c + R + 1])
    return density.astype(np.float32)


def heads_table(points: Union[np.ndarray, Sequence], shape) -> np.ndarray:
    """The head records of an image, float32 [N, 4] of (c, r, sigma, R): what ``gaussian_filter_density`` splats, kept
    instead of the map.  c, r = int(x), int(y), the pixel the delta goes to (out-of-image heads are dropped, as there;
    they still count as neighbours of the others); sigma the float32 rounding of the float64 ``knn_sigmas`` value;
    R = int(4 sigma64 + 0.5), from the float64 sigma and STORED: no later stage recomputes a radius from the rounded
    sigma.  sigma <= 0 (coincident heads) is a unit delta, R = 0."""
    h, w = _shape_of(shape)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    rows = []
    for (x, y), s in zip(pts, knn_sigmas(pts, (h, w))):
        if x < 0 or y < 0 or int(y) >= h or int(x) >= w:
            continue
        s = float(s)
        rows.append((int(x), int(y), s, int(4.0 * s + 0.5)) if s > 0 else (int(x), int(y), 0.0, 0))
    return np.asarray(rows, dtype=np.float32).reshape(-1, 4)


def heads_path(npy_path: str) -> str:
    """ground_truth/IMG_k.npy -> ground_truth/IMG_k.heads.npy, the sidecar of ``--heads``."""
    return os.path.splitext(npy_path)[0] + ".heads.npy"


def roi_path(npy_path: str) -> str:
    """ground_truth/IMG_k.npy -> ground_truth/IMG_k.roi.npy, the image's ROI mask: uint8 [H0, W0], 255 inside, 0
    outside, a in between the fraction a / 255."""
    return os.path.splitext(npy_path)[0] + ".roi.npy"


def density_map_gpu(points, h: int, w: int, device="cuda", max_radius: int = 0) -> torch.Tensor:
    """GPU density map [h, w] fp32 for points [[x, y], ...].  Not bitwise reproducible (fp32 atomics); measured on
    one MI355X against an fp64 reference (tests/test_gpu_density.py): the kNN sigma within 0.34 * 8 * 2^-24 relative,
    each head's contribution within 2.8 * 2^-24 * (1 + |a_y| + |a_x|) of itself, a the exponent of the Gaussian
    factor (about 8 at the edge of a footprint, more for a sigma below 1); the worst relative error of an element
    inside a footprint was 3.8e-7 for sigma-4 heads and 2.2e-6 over all cases.  The tests hold the kernel to
    20 * 2^-24 * (1 + |a_y| + |a_x|)."""
    from ..ops import _ext
    C = _ext.require()
    pts = torch.as_tensor(np.asarray(points, dtype=np.float32).reshape(-1, 2), device=device).contiguous()
    out = torch.zeros(h, w, dtype=torch.float32, device=device)
    n = pts.shape[0]
    if n == 0:
        return out
    sig = torch.empty(n, dtype=torch.float32, device=device)
    C.density_map(pts.data_ptr(), n, h, w, sig.data_ptr(), out.data_ptr(), max_radius, _ext.stream_ptr(device))
    return out


def load_sha_points(mat_path: str) -> np.ndarray:
    """ShanghaiTech GT_IMG_*.mat -> N x 2 (x=col, y=row) (reference :79-81)."""
    from scipy.io import loadmat
    mat = loadmat(mat_path)
    return np.asarray(mat["image_info"][0, 0][0, 0][0], dtype=np.float64)


def generate_dataset_density(root: str, parts=("train_data", "test_data"), use_gpu: bool = False,
                             heads: bool = False) -> int:
    """Offline driver (reference :58-92): writes ground_truth/IMG_k.npy next to images/IMG_k.jpg.  heads=True writes
    the head sidecars ground_truth/IMG_k.heads.npy (``heads_table``) INSTEAD: run it over a dataset whose maps exist, or
    after the plain run; without it exactly the files of the plain run are written."""
    from .dataset import imread
    count = 0
    for part in parts:
        for img_path in sorted(glob.glob(os.path.join(root, part, "images", "*.jpg"))):
            mat = img_path.replace(".jpg", ".mat").replace("images", "ground_truth").replace("IMG_", "GT_IMG_")
            img = imread(img_path)
            pts = load_sha_points(mat)
            out = img_path.replace(".jpg", ".npy").replace("images", "ground_truth")
            os.makedirs(os.path.dirname(out), exist_ok=True)
            if heads:
                np.save(heads_path(out), heads_table(pts, img.shape[:2]))
            elif use_gpu and torch.cuda.is_available():
                np.save(out, density_map_gpu(pts, img.shape[0], img.shape[1]).cpu().numpy())
            else:
                np.save(out, gaussian_filter_density(img, pts))
            count += 1
    return count


if __name__ == "__main__":  # pragma: no cover
    import argparse
    ap = argparse.ArgumentParser(description="generate geometry-adaptive density maps (ShanghaiTech layout)")
    ap.add_argument("root")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--heads", action="store_true",
                    help="write the head sidecars IMG_k.heads.npy (for train.py --gt-from-heads) instead of the maps")
    a = ap.parse_args()
    print(generate_dataset_density(a.root, use_gpu=a.gpu, heads=a.heads), "head tables" if a.heads else "maps", "written")
