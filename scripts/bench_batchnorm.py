"""Batch norm + ReLU, forward and backward, bf16: the native NHWC kernels (ops/batchnorm.py) next to stock
F.batch_norm + relu on a channels_last tensor.  Arms interleaved in one process, device events, median of --reps.
Achieved TB/s is over the bytes each native pass must move: forward 6 B per element (statistics read, apply read +
write), backward with ReLU 14 B (pass 1 reads dy, x, y; pass 2 reads them again and writes dx).

  python scripts/bench_batchnorm.py [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from can_distributed_pytorch_amd.ops import batchnorm as BN  # noqa: E402

SHAPES = [(8, 768, 1024, 64), (8, 384, 512, 128), (8, 96, 128, 512)]


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
    dev, eps, lines = "cuda", 1e-5, []
    for n, h, w, c in SHAPES:
        torch.manual_seed(0)
        x = (torch.randn(n, h, w, c, device=dev) * 2 + 1).to(torch.bfloat16)
        dy = torch.randn(n, h, w, c, device=dev).to(torch.bfloat16)
        gamma, beta = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)
        y, stats = BN.bn_forward(x, gamma, beta, None, None, True, eps, True)
        xs = x.permute(0, 3, 1, 2).detach().requires_grad_(True)             # NCHW view of channels_last memory
        gs, bs = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        ys = F.relu(F.batch_norm(xs, None, None, gs, bs, True, 0.1, eps))
        dys = dy.permute(0, 3, 1, 2)

        def stock_fwd():
            with torch.no_grad():
                F.relu(F.batch_norm(xs, None, None, gs, bs, True, 0.1, eps))

        arms = {"native_fwd": lambda: BN.bn_forward(x, gamma, beta, None, None, True, eps, True),
                "stock_fwd": stock_fwd,
                "native_bwd": lambda: BN.bn_backward(dy, x, y, gamma, stats, True, True),
                "stock_bwd": lambda: torch.autograd.grad(ys, [xs, gs, bs], dys, retain_graph=True)}
        t = {k: [] for k in arms}
        for rep in range(args.reps + 3):
            for k, fn in arms.items():                                       # interleaved
                us = timed(fn)
                if rep >= 3:
                    t[k].append(us)
        elems = x.numel()
        med = {k: statistics.median(v) for k, v in t.items()}
        rec = {"shape": [n, h, w, c], "reps": args.reps,
               **{k + "_us": round(v, 1) for k, v in med.items()},
               **{k + "_minmax_us": [round(min(v), 1), round(max(v), 1)] for k, v in t.items()},
               "native_fwd_TBps": round(6 * elems / med["native_fwd"] / 1e6, 2),
               "native_bwd_TBps": round(14 * elems / med["native_bwd"] / 1e6, 2)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del x, dy, y, xs, ys, dys
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
