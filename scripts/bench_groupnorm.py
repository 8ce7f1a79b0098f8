"""Group norm + ReLU, forward and backward, bf16: the native NHWC kernels (ops/groupnorm.py) in both forms next to stock
F.group_norm + relu on a channels_last tensor.  Arms interleaved in one process, device events around ten back-to-back
calls, median of --reps such windows after three warm-up rounds.  A form that cannot serve a shape (the resident tiles do not fit the LDS) is reported as null.
Effective GB/s is over the bytes the operation must move whatever the form: forward 4 B per element (read x, write y),
backward with ReLU 8 B (read dy, x, y, write dx); the streamed form moves 6 B and 14 B.

  python scripts/bench_groupnorm.py [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from can_distributed_pytorch_amd.ops import groupnorm as GN  # noqa: E402

# (N, H, W, C, G); the last one is the largest 512-channel map whose backward is resident
SHAPES = [(8, 96, 128, 512, 32), (8, 384, 512, 64, 64), (1, 96, 128, 512, 32), (8, 32, 32, 512, 32),
          (1, 768, 1024, 64, 64), (8, 24, 32, 512, 32)]
FORMS = {"streamed": GN.STREAMED, "resident": GN.RESIDENT}


INNER = 10                                  # calls per timed window: the smallest shapes take under 10 us a call


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / INNER  # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    dev, eps, lines = "cuda", 1e-5, []
    for n, h, w, c, groups in SHAPES:
        torch.manual_seed(0)
        x = (torch.randn(n, h, w, c, device=dev) * 2 + 1).to(torch.bfloat16)
        dy = torch.randn(n, h, w, c, device=dev).to(torch.bfloat16)
        gamma, beta = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)
        y, stats = GN.gn_forward(x, gamma, beta, groups, eps, True)
        xs = x.permute(0, 3, 1, 2).detach().requires_grad_(True)             # NCHW view of channels_last memory
        # stock group_norm wants the parameters in the activations' type
        gs, bs = (t.to(torch.bfloat16).requires_grad_(True) for t in (gamma, beta))
        ys = F.relu(F.group_norm(xs, groups, gs, bs, eps))
        dys = dy.permute(0, 3, 1, 2)

        def stock_fwd():
            with torch.no_grad():
                F.relu(F.group_norm(xs, groups, gs, bs, eps))

        arms = {"stock_fwd": stock_fwd,
                "stock_bwd": lambda: torch.autograd.grad(ys, [xs, gs, bs], dys, retain_graph=True)}
        planned = {}
        for name, form in FORMS.items():
            for bwd in (False, True):
                key = f"{name}_{'bwd' if bwd else 'fwd'}"
                if form == GN.RESIDENT and not GN.plan(x.shape, groups, bwd)["bundle"]:
                    continue
                if GN.plan(x.shape, groups, bwd)["form"] == form:
                    planned["bwd" if bwd else "fwd"] = name
                arms[key] = ((lambda f=form: GN.gn_backward(dy, x, y, gamma, stats, groups, True, form=f)) if bwd else
                             (lambda f=form: GN.gn_forward(x, gamma, beta, groups, eps, True, form=f)))
        t = {k: [] for k in arms}
        for rep in range(args.reps + 3):
            for k, fn in arms.items():                                       # interleaved
                us = timed(fn)
                if rep >= 3:
                    t[k].append(us)
        elems = x.numel()
        med = {k: statistics.median(v) for k, v in t.items()}
        keys = ["stock_fwd", "streamed_fwd", "resident_fwd", "stock_bwd", "streamed_bwd", "resident_bwd"]
        rec = {"shape": [n, h, w, c, groups], "reps": args.reps, "planned": planned,
               **{k + "_us": (round(med[k], 1) if k in med else None) for k in keys},
               **{k + "_minmax_us": [round(min(v), 1), round(max(v), 1)] for k, v in t.items()},
               **{k + "_GBps": round((8 if k.endswith("bwd") else 4) * elems / med[k] / 1e3) for k in keys if k in med}}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del x, dy, y, xs, ys, dys
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
