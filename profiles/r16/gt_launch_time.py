#!/usr/bin/env python
"""GPU time of the gt_from_heads launch (csrc/density.hip gt_from_heads_kernel) beside the image launch of the same
pack, in one process: 8 and 32 samples of 384 x 512, one crop per image, 200 and 3000 heads per image, s = 0.5, 1 and 2
(windows of (384, 512) / s at random offsets of 768 x 1024 sources, flips mixed).  The heads are the records
heads_table makes of clustered points (data/synthetic.py:synthetic_points): geometry-adaptive sigmas.  hipEvents around
ITERS back-to-back launches, best and median of REPS; one JSON line per arm.  C.gt_from_heads checks the host copy of
the head table before it launches, so back-to-back launches cannot go faster than that check: check_host_us is its
time alone (perf_counter around ITERS calls of C.gt_from_heads_check), and an arm whose launch time equals it is bound
by the host, not by the kernel.

usage: python profiles/r16/gt_launch_time.py  (from the repository root)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
while not os.path.isdir(os.path.join(ROOT, "can_distributed_pytorch_amd")):
    ROOT = os.path.dirname(ROOT)
sys.path.insert(0, ROOT)

from can_distributed_pytorch_amd.data.density import heads_table  # noqa: E402
from can_distributed_pytorch_amd.data.synthetic import synthetic_points  # noqa: E402
from can_distributed_pytorch_amd.ops import _ext  # noqa: E402
from can_distributed_pytorch_amd.ops.conv import dt_code  # noqa: E402
from can_distributed_pytorch_amd.ops.preprocess import PackedCollate  # noqa: E402

H, W, SH, SW = 384, 512, 768, 1024


def timed(launch, iters, reps):
    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            launch()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / iters)
    return round(min(us), 2), round(float(np.median(us)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    C = _ext.require()
    dev = torch.device("cuda")
    st = _ext.stream_ptr(dev)
    dt = dt_code(torch.bfloat16)
    rng = np.random.default_rng(0)
    gen = torch.Generator().manual_seed(0)
    for batch in (8, 32):
        imgs = [torch.from_numpy(rng.integers(0, 256, (SH, SW, 3), dtype=np.uint8)) for _ in range(batch)]
        x4 = torch.empty(batch, H, W, 4, dtype=torch.bfloat16, device=dev)
        for heads in (200, 3000):
            tabs = [torch.from_numpy(heads_table(synthetic_points(heads, SH, SW, gen).numpy(), (SH, SW)))
                    for _ in range(batch)]
            for s in (0.5, 1.0, 2.0):
                sh, sw = int(H / s + 0.5), int(W / s + 0.5)
                items = [(im, tab, torch.tensor([[int(rng.integers(0, SH - sh + 1)), int(rng.integers(0, SW - sw + 1)),
                                                  i % 2, sh, sw]])) for i, (im, tab) in enumerate(zip(imgs, tabs))]
                buf, meta = PackedCollate(crop=(H, W), crop_scale=True, gt_from_heads=True)(items)
                n, ho, wo, goff, doff = meta[:5]
                roff, hoff = doff + 64 * n, doff + 80 * n
                d = buf.to(dev)
                gt = d[goff:goff + 4 * n * (H // 8) * (W // 8)].view(torch.float32)

                def image():
                    C.preprocess_crop_scaled(d.data_ptr(), goff, d.data_ptr() + doff, buf.data_ptr() + doff, n,
                                             x4.data_ptr(), ho, wo, 8, dt, st)

                def render():
                    C.gt_from_heads(d.data_ptr() + hoff, d.data_ptr() + roff, d.data_ptr() + doff,
                                    buf.data_ptr() + hoff, meta[7], buf.data_ptr() + roff, buf.data_ptr() + doff, n,
                                    gt.data_ptr(), ho, wo, 8, st)

                t0 = time.perf_counter()
                for _ in range(a.iters):
                    C.gt_from_heads_check(buf.data_ptr() + hoff, meta[7], buf.data_ptr() + roff, buf.data_ptr() + doff,
                                          n, ho, wo, 8)
                check_us = round((time.perf_counter() - t0) * 1e6 / a.iters, 2)
                ib, im_ = timed(image, a.iters, a.reps)
                rb, rm = timed(render, a.iters, a.reps)
                sig = torch.cat(tabs)[:, 2]
                print(json.dumps(dict(batch=batch, heads_per_image=heads, s=s, window=[sh, sw],
                                      sigma_median=round(float(sig.median()), 2), radius_max=int(torch.cat(tabs)[:, 3].max()),
                                      gt_from_heads_us_best=rb, gt_from_heads_us_median=rm, image_us_best=ib,
                                      image_us_median=im_, check_host_us=check_us, pack_mb=round(buf.numel() / 1e6, 2),
                                      heads_kb=round(16 * meta[7] / 1e3, 1))), flush=True)


if __name__ == "__main__":
    main()
