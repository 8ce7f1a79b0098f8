#!/usr/bin/env python
"""GPU time of the scaled crop launch (csrc/preprocess.hip preprocess_crop_scaled_kernel) beside the crop launch and
the resize launch at the same output size: batch x HxW NHWC4 bf16 from packed uint8 RGB images already on the device
(the protocol of scripts/prof/crop_launch_time.py).  Scaled arms: windows of (H, W) / s at random offsets of 2H x 2W
sources, flips mixed, s = 0.5 (the window is the source), 1 and 2.  hipEvents around ITERS back-to-back launches, best
and median of REPS; one JSON line per arm.

usage: python profiles/r13/scaled_launch_time.py [--batch 8] [--size 384x512]  (from the repository root)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
while not os.path.isdir(os.path.join(ROOT, "can_distributed_pytorch_amd")):
    ROOT = os.path.dirname(ROOT)
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

    def scaled(srcs, s):
        sh, sw = int(h / s + 0.5), int(w / s + 0.5)
        return PackedCollate(crop=(h, w), crop_scale=True)(
            [(im, gt1[None], torch.tensor([[int(rng.integers(0, im.shape[0] - sh + 1)),
                                            int(rng.integers(0, im.shape[1] - sw + 1)), i % 2, sh, sw]]))
             for i, im in enumerate(srcs)])

    small, big = images(h, w), images(2 * h, 2 * w)
    packs = {
        "resize": PackedCollate()([(im, gt1, i % 2) for i, im in enumerate(small)]),
        "crop_same_size": PackedCollate(crop=(h, w))([(im, gt1[None], torch.tensor([[0, 0, i % 2]]))
                                                      for i, im in enumerate(small)]),
        "crop_of_2x_source": PackedCollate(crop=(h, w))(
            [(im, gt1[None], torch.tensor([[int(rng.integers(0, h + 1)), int(rng.integers(0, w + 1)), i % 2]]))
             for i, im in enumerate(big)]),
        "scaled_same_size_s1": scaled(small, 1.0),
        "scaled_of_2x_source_s0.5": scaled(big, 0.5),
        "scaled_of_2x_source_s1": scaled(big, 1.0),
        "scaled_of_2x_source_s2": scaled(big, 2.0),
    }
    x4 = torch.empty(a.batch, h, w, 4, dtype=torch.bfloat16, device=dev)
    dt = dt_code(torch.bfloat16)
    for name, (buf, meta) in packs.items():
        n, ho, wo, goff, doff = meta[:5]
        d = buf.to(dev)
        desc = d[doff:].view(torch.int64)
        if len(meta) == 7:
            def launch():
                C.preprocess_crop_scaled(d.data_ptr(), goff, desc.data_ptr(), buf.data_ptr() + doff, n, x4.data_ptr(),
                                         ho, wo, 8, dt, st)
        elif len(meta) == 6:
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
