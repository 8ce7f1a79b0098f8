"""Adaptive average pool and bilinear resize, forward and backward, bf16: the native NHWC kernels (ops/resample.py)
next to stock F.adaptive_avg_pool2d / F.interpolate on a channels_last tensor.  Arms interleaved in one process,
device events, median of --reps.  Achieved GB/s is over the bytes the contract must move: every element of the call's
input read once and every element of its output written once, 2 B each (the tap tables and the separable pool's fp32
row sums are the implementation's own traffic and are not counted).

  python scripts/bench_resample.py [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from can_distributed_pytorch_amd.ops import resample as RS  # noqa: E402

# (op, input N H W C, output oh ow, align_corners): the context module's scales on its feature map and back, the
# VGG-19 point-loss networks' x2, one downscale
CASES = [("pool", (8, 96, 128, 512), (s, s), None) for s in (1, 2, 3, 6)] + \
        [("resize", (8, s, s, 512), (96, 128), True) for s in (1, 2, 3, 6)] + \
        [("resize", (8, 48, 64, 512), (96, 128), False), ("resize", (8, 96, 128, 512), (48, 64), False)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3          # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    dev, lines = "cuda", []
    for op, shape, (oh, ow), align in CASES:
        torch.manual_seed(0)
        n, h, w, c = shape
        x = torch.randn(*shape, device=dev).to(torch.bfloat16)
        dy = torch.randn(n, oh, ow, c, device=dev).to(torch.bfloat16)
        xs = x.permute(0, 3, 1, 2).detach().requires_grad_(True)            # NCHW view of channels_last memory
        dys = dy.permute(0, 3, 1, 2)
        if op == "pool":
            stock = lambda t: F.adaptive_avg_pool2d(t, (oh, ow))
            nat_f = lambda: RS.adaptive_avg_pool(x, oh, ow)
            nat_b = lambda: RS.adaptive_avg_pool_backward(dy, h, w)
            plan = RS.pool_plan(shape, oh, ow)
        else:
            stock = lambda t: F.interpolate(t, size=(oh, ow), mode="bilinear", align_corners=align)
            nat_f = lambda: RS.resize_bilinear(x, oh, ow, align)
            nat_b = lambda: RS.resize_bilinear_backward(dy, h, w, align)
            plan = RS.resize_plan(shape, oh, ow)
        ys = stock(xs)

        def stock_fwd():
            with torch.no_grad():
                stock(xs)

        arms = {"native_fwd": nat_f, "stock_fwd": stock_fwd, "native_bwd": nat_b,
                "stock_bwd": lambda: torch.autograd.grad(ys, xs, dys, retain_graph=True)}
        t = {k: [] for k in arms}
        for rep in range(args.reps + 3):
            for k, fn in arms.items():                                       # interleaved
                us = timed(fn)
                if rep >= 3:
                    t[k].append(us)
        moved = 2 * (x.numel() + dy.numel())
        med = {k: statistics.median(v) for k, v in t.items()}
        rec = {"op": op, "in": list(shape), "out": [oh, ow], "align_corners": align, "reps": args.reps, "plan": plan,
               **{k + "_us": round(v, 1) for k, v in med.items()},
               **{k + "_minmax_us": [round(min(v), 1), round(max(v), 1)] for k, v in t.items()},
               "native_fwd_GBps": round(moved / med["native_fwd"] / 1e3, 1),
               "native_bwd_GBps": round(moved / med["native_bwd"] / 1e3, 1),
               "fwd_vs_stock": round(med["stock_fwd"] / med["native_fwd"], 2),
               "bwd_vs_stock": round(med["stock_bwd"] / med["native_bwd"], 2)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del x, dy, xs, ys, dys
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
