#!/usr/bin/env python
"""Device time of the gradient-norm pass (elementwise.hip grad_norm_partial_kernel + grad_norm_final_kernel) against the
fp16 overflow check (grad_nonfinite_kernel) over the model's gradient arena, and the whole native step at batch 1 with
gradient accumulation and clipping on and off.

    python scripts/bench_accum_clip.py --out profiles/r8/accum_clip.jsonl
    python scripts/bench_accum_clip.py --whole-step --out profiles/r8/accum_clip.jsonl

Kernel arms: one NativeStepper's arena; the two arms alternate within the process (``--rounds`` rounds of ``--launches``
back-to-back calls per arm between two device events).  Both read the arena's parameters once; the bytes counted are
those reads.  Whole step: 768x1024, batch 1, bf16, eager; SGD and AdamW, accum_steps 1 against 4, clipping off against
max_norm 1; every arm is its own stepper and the arms alternate round by round.  One JSON line per arm is printed and
appended to ``--out``."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def kernel_arms(args):
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    st = NativeStepper(dev, dtype=args.dtype, graph=False, clip_grad_norm=1.0)
    st.arena.grad.normal_()
    n = sum(p.numel() for p in st.params)
    stream = torch.cuda.current_stream().cuda_stream
    C, ex = st.C, st.ex
    arms = {
        "grad_norm": (lambda: ex.grad_norm(1.0, 1.0, st.flags), 4 * n, 2,
                      "both stages: per-chunk double partials, then the per-parameter and global sums"),
        "grad_nonfinite": (lambda: C.grad_nonfinite(st.arena.grad.data_ptr(), st.arena.numel,
                                                    st.flags.data_ptr() + 8, stream), 4 * st.arena.numel, 1,
                           "the fp16 step's overflow check (reads the slots' padding too)"),
    }
    for fn, *_ in arms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, (fn, *_) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.launches)
    assert float(st.flags[2]) == 0 and st.clip_coef() < 1.0
    for name, (_, nbytes, per_call, note) in arms.items():
        v = sorted(ms[name])
        med = v[len(v) // 2]
        emit({"kind": "norm_kernel", "arm": name, "params": n, "arena_floats": st.arena.numel, "bytes": nbytes,
              "calls": args.rounds * args.launches, "device_launches_per_call": per_call,
              "us_median": round(med * 1e3, 2), "us_min": round(v[0] * 1e3, 2), "us_max": round(v[-1] * 1e3, 2),
              "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3), "note": note}, args.out)


def whole_step(args):
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    dev = torch.device("cuda", 0)
    img, gt = make_synthetic_batch(1, 768, 1024, seed=0, device=dev)
    st = {}
    for name, lr in (("sgd", 1e-7), ("adamw", 1e-5)):
        for k in (1, 4):
            for clip in (0.0, 1.0):
                torch.manual_seed(0)
                s = NativeStepper(dev, dtype=args.dtype, lr=lr, batch=1, graph=False, optimizer=name, accum_steps=k,
                                  clip_grad_norm=clip)
                for _ in range(args.warmup * 4):
                    s.step(img, gt)
                st[(name, k, clip)] = s
    torch.cuda.synchronize()
    ips = {k: [] for k in st}
    for _ in range(args.rounds):
        for key, s in st.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step(img, gt)
            torch.cuda.synchronize()
            ips[key].append(args.steps / (time.perf_counter() - t0))
    for (name, k, clip), v in ips.items():
        v = sorted(v)
        emit({"kind": "whole_step", "optimizer": name, "accum_steps": k, "clip_grad_norm": clip, "dtype": args.dtype,
              "batch": 1, "size": "768x1024", "graph": False, "micro_steps": args.rounds * args.steps,
              "img_per_s_median": round(v[len(v) // 2], 2), "img_per_s_min": round(v[0], 2),
              "img_per_s_max": round(v[-1], 2), "finite": not st[(name, k, clip)].nonfinite()}, args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=25, help="kernel arms: calls per arm and round")
    ap.add_argument("--steps", type=int, default=40, help="--whole-step: micro-steps per arm and round (a multiple of 4)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--whole-step", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    (whole_step if args.whole_step else kernel_arms)(args)


if __name__ == "__main__":
    main()
