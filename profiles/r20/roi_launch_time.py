#!/usr/bin/env python
"""GPU time of the two launches the ROI-mask feature adds to a training step, each beside the launch it rides with
(the protocol of profiles/r13/scaled_launch_time.py: REPS rounds of ITERS back-to-back launches, hipEvents around a
round, the arms of a table taking turns; best and median, one JSON line per arm).

roi_*:   C.roi_weights (csrc/preprocess.hip roi_weights_kernel) beside the image launch of the same pack, batch x HxW
         from packed uint8 RGBA images already on the device: unscaled crops, and windows of (H, W) / s for s = 0.5, 1, 2.
         Also the pack's bytes against the same pack with 3-channel images (the extra H2D copy).
head_*:  C.head_train with the weight plane (head_train_kernel<DT, true>) beside the unweighted launch, P = batch x
         H/8 x W/8 pixels and the default benchmark's 8 x 96 x 128.

usage: python profiles/r20/roi_launch_time.py [--batch 8] [--size 384x512]  (from the repository root)
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


def timed(arms, iters, reps):
    us = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: (round(min(v), 2), round(float(np.median(v)), 2)) for k, v in us.items()}


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
    dt = dt_code(torch.bfloat16)
    gt1 = torch.rand(1, 1, h // 8, w // 8)
    big = []
    for _ in range(a.batch):                      # 2H x 2W sources: noise colours, a mask of 32 x 32 blocks as alpha
        im = rng.integers(0, 256, (2 * h, 2 * w, 4), dtype=np.uint8)
        im[:, :, 3] = np.kron(rng.integers(0, 2, (2 * h // 32, 2 * w // 32), dtype=np.uint8) * 255,
                              np.ones((32, 32), dtype=np.uint8))
        big.append(torch.from_numpy(im))
    x4 = torch.empty(a.batch, h, w, 4, dtype=torch.bfloat16, device=dev)
    gt2 = torch.empty(a.batch, 2, h // 8, w // 8, dtype=torch.float32, device=dev)
    for name, s in (("crop", None), ("scaled_s0.5", 0.5), ("scaled_s1", 1.0), ("scaled_s2", 2.0)):
        items = []
        for i, im in enumerate(big):
            if s is None:
                win = [int(rng.integers(0, im.shape[0] - h + 1)), int(rng.integers(0, im.shape[1] - w + 1)), i % 2]
            else:
                sh, sw = int(h / s + 0.5), int(w / s + 0.5)
                win = [int(rng.integers(0, im.shape[0] - sh + 1)), int(rng.integers(0, im.shape[1] - sw + 1)), i % 2,
                       sh, sw]
            items.append((im, gt1, torch.tensor([win])))
        collate = PackedCollate(crop=(h, w), crop_scale=s is not None)
        buf, meta = collate(items)
        buf3, _ = collate([(im[:, :, :3].contiguous(), g, win) for im, g, win in items])
        n, ho, wo, goff, doff = meta[:5]
        d = buf.to(dev)
        image = C.preprocess_crop if s is None else C.preprocess_crop_scaled

        def launch_image():
            image(d.data_ptr(), goff, d.data_ptr() + doff, buf.data_ptr() + doff, n, x4.data_ptr(), ho, wo, 8, dt, st)

        def launch_roi():
            C.roi_weights(d.data_ptr(), goff, d.data_ptr() + doff, buf.data_ptr() + doff, n, d.data_ptr() + goff,
                          gt2.data_ptr(), ho, wo, 8, st)

        for k, (best, med) in timed({"image": launch_image, "roi": launch_roi}, a.iters, a.reps).items():
            print(json.dumps(dict(arm=f"roi_{name}_{k}", batch=a.batch, out=[h, w], us_best=best, us_median=med,
                                  pack_bytes_rgba=buf.numel(), pack_bytes_rgb=buf3.numel())), flush=True)

    for n, hh, ww in ((a.batch, h // 8, w // 8), (8, 96, 128)):
        P = n * hh * ww
        g = torch.Generator().manual_seed(P)
        y = torch.relu(torch.randn(P, 64, generator=g)).to(torch.bfloat16).to(dev)
        wgt, b = (0.1 * torch.randn(64, generator=g)).to(dev), torch.tensor([0.3], device=dev)
        gt, m = torch.rand(P, generator=g).to(dev), torch.rand(P, generator=g).to(dev)
        nblk = max(1, min(1024, (P * 8 + 255) // 256))
        et, dy = torch.empty(P, device=dev), torch.empty(P, 64, dtype=torch.bfloat16, device=dev)
        part, dw, db = torch.empty(nblk, 66, device=dev), torch.empty(64, device=dev), torch.empty(1, device=dev)
        loss, nf = torch.empty(1, device=dev), torch.empty(1, device=dev)

        def head(wt):
            C.head_train(y.data_ptr(), wgt.data_ptr(), b.data_ptr(), gt.data_ptr(), et.data_ptr(), dy.data_ptr(),
                         part.data_ptr(), nblk, dw.data_ptr(), db.data_ptr(), loss.data_ptr(), P, 1.0, 0.0, 0,
                         nf.data_ptr(), dt, st, 0, 0, wt)

        res = timed({"unweighted": lambda: head(0), "weighted": lambda: head(m.data_ptr())}, a.iters, a.reps)
        for k, (best, med) in res.items():
            print(json.dumps(dict(arm=f"head_{k}", pixels=P, shape=[n, hh, ww], us_best=best, us_median=med)),
                  flush=True)


if __name__ == "__main__":
    main()
