#!/usr/bin/env python
"""How much count the point-sampled ground truth of a scaled crop loses or gains (CPU, no GPU involved).

A 384 x 512 crop at scale s resamples a window of (384, 512) / s.  The window holds unit-mass Gaussians of one sigma
(2, 4 or 8 px), centres uniform at sub-pixel positions at least 4 sigma + 8 px inside it.  The ground truth is
density_to_gt_scaled's [48, 64] map; the figure is |sum(gt) - sum(window)| / sum(window): over a window of 200 heads
(mean and max of 8 windows) and over a window of ONE head (mean and max of 200 positions), the latter being what a
sparse crop sees.  One line per (sigma, s); s = 1 is the unscaled rule's own value.

usage: python profiles/r13/count_deviation.py  (from the repository root)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
while not os.path.isdir(os.path.join(ROOT, "can_distributed_pytorch_amd")):
    ROOT = os.path.dirname(ROOT)
sys.path.insert(0, ROOT)

from can_distributed_pytorch_amd.data.dataset import density_to_gt_scaled, scaled_window  # noqa: E402

CH, CW, D = 384, 512, 8


def window_of(points, sigma, sh, sw):
    """Sum of unit-mass Gaussians (normalised over the pixels they cover, radius 4 sigma), float64."""
    out = np.zeros((sh, sw), dtype=np.float64)
    r = int(np.ceil(4 * sigma))
    for cy, cx in points:
        y0, x0 = int(np.floor(cy)) - r, int(np.floor(cx)) - r
        ys, xs = np.arange(y0, y0 + 2 * r + 2), np.arange(x0, x0 + 2 * r + 2)
        g = np.exp(-((ys[:, None] - cy) ** 2 + (xs[None] - cx) ** 2) / (2.0 * sigma * sigma))
        out[y0:y0 + 2 * r + 2, x0:x0 + 2 * r + 2] += g / g.sum()
    return out


def deviation(rng, sigma, s, heads):
    sh, sw = scaled_window(4 * CH, 4 * CW, CH, CW, s)
    m = 4 * sigma + 8
    pts = np.stack([rng.uniform(m, sh - m, heads), rng.uniform(m, sw - m, heads)], axis=1)
    win = window_of(pts, sigma, sh, sw).astype(np.float32)
    gt = density_to_gt_scaled(win, CH, CW, D, False)
    return abs(float(gt.sum(dtype=np.float64)) - float(win.sum(dtype=np.float64))) / float(win.sum(dtype=np.float64))


def main():
    print("sigma  s     window     stride  200 heads: mean   max      1 head: mean   max")
    for sigma in (2.0, 4.0, 8.0):
        for s in (0.5, 0.75, 1.0, 1.33, 2.0):
            rng = np.random.default_rng(int(sigma * 100 + s * 1000))
            sh, sw = scaled_window(4 * CH, 4 * CW, CH, CW, s)
            many = [deviation(rng, sigma, s, 200) for _ in range(8)]
            one = [deviation(rng, sigma, s, 1) for _ in range(200)]
            print(f"{sigma:4.0f}  {s:4.2f}  {sh:4d}x{sw:<4d}  {D / s:5.2f}   {np.mean(many):14.4f}  {np.max(many):6.4f}"
                  f"   {np.mean(one):12.4f}  {np.max(one):6.4f}", flush=True)


if __name__ == "__main__":
    main()
