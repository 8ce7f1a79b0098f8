#!/usr/bin/env python
"""GPU time of the crop launch (csrc/preprocess.hip preprocess_crop_kernel) beside the resize launch
(preprocess_resample_kernel) at the same output size: batch x HxW NHWC4 bf16 from packed uint8 RGB images already on
the device.  Arms: resize of HxW sources (scale 1: four taps per pixel), crop of the same HxW sources (the window is
the image) and crop of 2H x 2W sources at random offsets with flips.  hipEvents around ITERS back-to-back launches,
best and median of REPS; one JSON line per arm.

usage: python scripts/prof/crop_launch_time.py [--batch 8] [--size 384x512]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from can_distributed_pytorch_amd.ops import _ext  # noqa: E402
from can_distributed_pytorch_amd.ops.conv import dt_code  # noqa: E402
from can_distributed_pytorch_amd.ops.preprocess import PackedCollate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", default="384x512")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    h, w = (int(v) for v in a.size.lower().split("x"))
    C = _ext.require()
    dev = torch.device("cuda")
    st = _ext.stream_ptr(dev)
    rng = np.random.default_rng(0)
    gt1 = torch.zeros(1, h // 8, w // 8)

    def images(hh, ww):
        return [torch.from_numpy(rng.integers(0, 256, (hh, ww, 3), dtype=np.uint8)) for _ in range(a.batch)]

    small, big = images(h, w), images(2 * h, 2 * w)
    packs = {
        "resize": PackedCollate()([(im, gt1, i % 2) for i, im in enumerate(small)]),
        "crop_same_size": PackedCollate(crop=(h, w))([(im, gt1[None], torch.tensor([[0, 0, i % 2]]))
                                                      for i, im in enumerate(small)]),
        "crop_of_2x_source": PackedCollate(crop=(h, w))(
            [(im, gt1[None], torch.tensor([[int(rng.integers(0, h + 1)), int(rng.integers(0, w + 1)), i % 2]]))
             for i, im in enumerate(big)]),
    }
    x4 = torch.empty(a.batch, h, w, 4, dtype=torch.bfloat16, device=dev)
    dt = dt_code(torch.bfloat16)
    for name, (buf, meta) in packs.items():
        n, ho, wo, goff, doff = meta[:5]
        d = buf.to(dev)
        desc = d[doff:].view(torch.int64)
        if len(meta) == 6:
            def launch():
                C.preprocess_crop(d.data_ptr(), goff, desc.data_ptr(), buf.data_ptr() + doff, n, x4.data_ptr(), ho, wo,
                                  8, dt, st)
        else:
            def launch():
                C.preprocess_batch(d.data_ptr(), 0, desc.data_ptr(), n, x4.data_ptr(), 0, ho, wo, 8, dt, st)
        for _ in range(10):
            launch()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                launch()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        out_mb = x4.numel() * 2 / 1e6
        print(json.dumps(dict(arm=name, batch=a.batch, out=[h, w], us_best=round(min(us), 2),
                              us_median=round(float(np.median(us)), 2), out_gbps_best=round(out_mb / min(us) * 1e3, 1))),
              flush=True)


if __name__ == "__main__":
    main()
