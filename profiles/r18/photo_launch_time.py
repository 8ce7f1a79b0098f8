#!/usr/bin/env python
"""GPU time of the photo launch (csrc/preprocess.hip, the PHOTO instantiations behind C.preprocess_crop_photo) beside the
plain launch of the same pack: batch x HxW NHWC4 bf16 from packed uint8 RGB images already on the device (the protocol
of profiles/r13/scaled_launch_time.py).  Crop arms: windows at random offsets of 2H x 2W sources, flips mixed.  Scaled
arms: windows of (H, W) / s, s = 0.5 (the window is the source), 1 and 2.  Photo arms carry one real tone table per
sample, every second sample gray; the *_noise arms put the same tables on uniform random bytes and the *_flat arms on a
smooth image (neighbouring lanes then read the same or neighbouring table entries), which brackets the LDS bank
conflicts of the data-dependent lookup.  The plain and the photo arm of a pack are timed in turns (REPS rounds of ITERS
back-to-back launches each, hipEvents around a round); best and median, one JSON line per arm.

usage: python profiles/r18/photo_launch_time.py [--batch 8] [--size 384x512]  (from the repository root)
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

from can_distributed_pytorch_amd.data.transforms import photo_table  # noqa: E402
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
    gt1 = torch.zeros(1, 1, h // 8, w // 8)
    rows = np.zeros((a.batch, 257), dtype=np.float32)
    for i in range(a.batch):
        rows[i, :256] = photo_table(rng.uniform(-0.2, 0.2), 1.3 ** rng.uniform(-1, 1), 1.5 ** rng.uniform(-1, 1))
        rows[i, 256] = i % 2
    rows = torch.from_numpy(rows)

    def noise(hh, ww):
        return [torch.from_numpy(rng.integers(0, 256, (hh, ww, 3), dtype=np.uint8)) for _ in range(a.batch)]

    def flat(hh, ww):                              # a smooth ramp: neighbouring pixels differ by at most one level
        y, x = np.mgrid[0:hh, 0:ww]
        base = (y * 97.0 / hh + x * 131.0 / ww)
        return [torch.from_numpy(np.stack([(base + 17 * c + 5 * i) % 256 for c in range(3)], 2).astype(np.uint8))
                for i in range(a.batch)]

    def items(srcs, s):
        out = []
        for i, im in enumerate(srcs):
            if s is None:
                win = [int(rng.integers(0, im.shape[0] - h + 1)), int(rng.integers(0, im.shape[1] - w + 1)), i % 2]
            else:
                sh, sw = int(h / s + 0.5), int(w / s + 0.5)
                win = [int(rng.integers(0, im.shape[0] - sh + 1)), int(rng.integers(0, im.shape[1] - sw + 1)), i % 2,
                       sh, sw]
            out.append((im, gt1, torch.tensor([win]), rows[i:i + 1]))
        return out

    x4 = torch.empty(a.batch, h, w, 4, dtype=torch.bfloat16, device=dev)
    dt = dt_code(torch.bfloat16)
    for content, make in (("noise", noise), ("flat", flat)):
        big = make(2 * h, 2 * w)
        for name, s in (("crop", None), ("scaled_s0.5", 0.5), ("scaled_s1", 1.0), ("scaled_s2", 2.0)):
            its = items(big, s)
            buf, meta = PackedCollate(crop=(h, w), crop_scale=s is not None, photo=True)(its)
            n, ho, wo, goff, doff, poff = *meta[:5], meta[8]
            d = buf.to(dev)
            plain = C.preprocess_crop if s is None else C.preprocess_crop_scaled

            def launch_plain():
                plain(d.data_ptr(), goff, d.data_ptr() + doff, buf.data_ptr() + doff, n, x4.data_ptr(), ho, wo, 8, dt, st)

            def launch_photo():
                C.preprocess_crop_photo(d.data_ptr(), goff, d.data_ptr() + doff, buf.data_ptr() + doff, n,
                                        x4.data_ptr(), ho, wo, 8, dt, st, d.data_ptr() + poff, buf.data_ptr() + poff,
                                        int(s is not None))

            arms = {"plain": launch_plain, "photo": launch_photo}
            us = {k: [] for k in arms}
            for fn in arms.values():
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.reps):
                for k, fn in arms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    us[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
            for k in arms:
                print(json.dumps(dict(arm=f"{name}_{content}_{k}", batch=a.batch, out=[h, w],
                                      us_best=round(min(us[k]), 2), us_median=round(float(np.median(us[k])), 2))),
                      flush=True)


if __name__ == "__main__":
    main()
