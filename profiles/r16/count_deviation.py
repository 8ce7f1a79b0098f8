#!/usr/bin/env python
"""The count a scaled crop's ground truth loses or gains when it is rendered from head records (heads_to_gt), with the
protocol of profiles/r13/count_deviation.py (CPU, no GPU involved).

A 384 x 512 crop at scale s covers a window of (384, 512) / s.  The window holds heads of one sigma (2, 4 or 8 px) at
uniform sub-pixel positions at least 4 sigma + 8 px inside it; a head is the record (int(x), int(y), sigma,
int(4 sigma + 0.5)) of data/density.py:heads_table and the window's mass is the sum of the reference generator's map
over it, built here from the records in float64 by outer products.  The figure is |sum(gt) - sum(window)| /
sum(window) of the fp32 [48, 64] ground truth: over a window of 200 heads (mean and max of 8 windows) and over a window
of ONE head (mean and max of 200 positions).  One line per (sigma, s).

usage: python profiles/r16/count_deviation.py  (from the repository root)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
while not os.path.isdir(os.path.join(ROOT, "can_distributed_pytorch_amd")):
    ROOT = os.path.dirname(ROOT)
sys.path.insert(0, ROOT)

from can_distributed_pytorch_amd.data.dataset import scaled_window  # noqa: E402
from can_distributed_pytorch_amd.data.transforms import heads_to_gt  # noqa: E402

CH, CW, D = 384, 512, 8


def window_mass(records, sh, sw):
    """Sum over the window's pixels of the reference map of the records, float64 (every footprint lies inside)."""
    out = np.zeros((sh, sw), dtype=np.float64)
    for c, r, sigma, R in records:
        t = np.arange(-int(R), int(R) + 1, dtype=np.float64)
        k = np.exp(-(t * t) / (2.0 * float(np.float32(sigma)) ** 2))
        k /= k.sum()
        out[int(r) - int(R):int(r) + int(R) + 1, int(c) - int(R):int(c) + int(R) + 1] += np.outer(k, k)
    return float(out.sum())


def deviation(rng, sigma, s, heads):
    sh, sw = scaled_window(4 * CH, 4 * CW, CH, CW, s)
    m = 4 * sigma + 8
    ys, xs = rng.uniform(m, sh - m, heads), rng.uniform(m, sw - m, heads)
    rec = np.asarray([(int(x), int(y), sigma, int(4.0 * sigma + 0.5)) for y, x in zip(ys, xs)], dtype=np.float32)
    gt = heads_to_gt(rec, sh, sw, (0, 0, sh, sw), CH, CW, D, False)
    mass = window_mass(rec, sh, sw)
    return abs(float(gt.sum(dtype=np.float64)) - mass) / mass


def main():
    print("sigma  s     window     200 heads: mean   max        1 head: mean   max")
    for sigma in (2.0, 4.0, 8.0):
        for s in (0.5, 0.75, 1.0, 1.33, 2.0):
            rng = np.random.default_rng(int(sigma * 100 + s * 1000))
            sh, sw = scaled_window(4 * CH, 4 * CW, CH, CW, s)
            many = [deviation(rng, sigma, s, 200) for _ in range(8)]
            one = [deviation(rng, sigma, s, 1) for _ in range(200)]
            print(f"{sigma:4.0f}  {s:4.2f}  {sh:4d}x{sw:<4d}  {np.mean(many):14.2e}  {np.max(many):8.2e}"
                  f"   {np.mean(one):12.2e}  {np.max(one):8.2e}", flush=True)


if __name__ == "__main__":
    main()
