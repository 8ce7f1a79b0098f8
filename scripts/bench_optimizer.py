#!/usr/bin/env python
"""Device time of the fused optimizer step (elementwise.hip pack_multi_kernel<DT, OPT>: the update over the fp32 arena
+ the 16-bit weight packs, one launch) for SGD-momentum, SGD + weight decay and Adam, and of the whole native step with
Adam against SGD.

    python scripts/bench_optimizer.py --out profiles/r7/optimizer_step.jsonl
    python scripts/bench_optimizer.py --whole-step --out profiles/r7/optimizer_step.jsonl

Kernel arms: one CANNetExecutor arena; the arms alternate within the process (``--rounds`` rounds of ``--launches``
back-to-back launches per arm between two device events).  Bytes moved per launch are counted here: masters read +
written, gradients read, each optimizer state arena read + written, the packs written.  A fourth, diagnostic arm runs
the stand-alone Adam kernel over the same arena (the same arithmetic as a plain float4 stream, without the LDS transpose
and the packs).  The EMA arms (``sgd_ema``, ``adam_ema``: the same launches with the EMA arena updated inside them;
``ema_flat``: the stand-alone EMA kernel, which re-reads the masters) run interleaved with the others; each EMA arena adds
one read and one write of the arena to the count.  ``--whole-step`` runs SGD and Adam with and without EMA.  One JSON
line per arm is printed and appended to ``--out``."""
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
    from can_distributed_pytorch_amd.engine.native import ACT_DTYPES
    from can_distributed_pytorch_amd.models import CANNet
    from can_distributed_pytorch_amd.ops.executor import CANNetExecutor
    from can_distributed_pytorch_amd.utils.flat import FlatArena
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = CANNet(backend="hip").to(dev)
    ex = CANNetExecutor(model, dtype=ACT_DTYPES[args.dtype])
    params = list(model.parameters())
    arena = FlatArena(params, dev, order=ex.grad_ready_order())
    arena.grad.normal_()
    mom, mom2 = torch.zeros_like(arena.data), torch.zeros_like(arena.data)
    t = torch.zeros(1, dtype=torch.int32, device=dev)
    ema = arena.data.clone()
    et = torch.zeros(1, dtype=torch.int32, device=dev)
    ekw = dict(ema=ema, ema_t=et, ema_decay=0.999, ema_warmup=True)
    flags = torch.zeros(4, device=dev)
    lr_dev = torch.full((1,), 1e-9, device=dev)
    ex.refresh_packs(force=True)
    n = sum(p.numel() for p in params)
    pack_bytes = 2 * (ex.ctx2cat_fwd.numel() + ex.ctx2cat_dgr.numel() +
                      sum(x.numel() for pk in ex.packs.values() for x in pk if x is not None))
    common = dict(flags=flags, lr_dev=lr_dev)
    nf = arena.data.numel()
    stream = torch.cuda.current_stream().cuda_stream

    def fused_bytes(states, ema_arenas=0):
        return 4 * n * (2 + 1 + 2 * states + 2 * ema_arenas) + pack_bytes

    # arm: (launch, bytes moved, device launches per call, note)
    arms = {
        "sgd": (lambda: ex.opt_step(arena.data, arena.grad, mom, 1e-9, 1.0, optimizer="sgd", **common),
                fused_bytes(1), 1, ""),
        "sgd_wd": (lambda: ex.opt_step(arena.data, arena.grad, mom, 1e-9, 1.0, optimizer="sgd", weight_decay=5e-4,
                                       **common), fused_bytes(1), 1, ""),
        "adam": (lambda: ex.opt_step(arena.data, arena.grad, mom, 1e-9, 1.0, optimizer="adam", mom2=mom2, step=t,
                                     **common), fused_bytes(2), 2, "includes the one-thread step-count launch"),
        # diagnostic: the same per-element arithmetic as a plain float4 stream, no LDS transpose and no packs
        "adam_flat": (lambda: ex.C.adam(arena.data.data_ptr(), mom.data_ptr(), mom2.data_ptr(), arena.grad.data_ptr(),
                                        nf, 1e-9, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, 0, t.data_ptr(), flags.data_ptr(),
                                        lr_dev.data_ptr(), stream), 4 * nf * 7, 2,
                      "stand-alone adam_kernel over the arena, no packs; includes the step-count launch"),
        "sgd_ema": (lambda: ex.opt_step(arena.data, arena.grad, mom, 1e-9, 1.0, optimizer="sgd", **ekw, **common),
                    fused_bytes(1, 1), 2, "includes the one-thread count launch"),
        "adam_ema": (lambda: ex.opt_step(arena.data, arena.grad, mom, 1e-9, 1.0, optimizer="adam", mom2=mom2, step=t,
                                         **ekw, **common), fused_bytes(2, 1), 2,
                     "includes the one-thread count launch (both counts in one)"),
        # the two-launch alternative's second launch: masters re-read, EMA read + written
        "ema_flat": (lambda: ex.C.ema(ema.data_ptr(), arena.data.data_ptr(), nf, 0.999, 1, 0, et.data_ptr(),
                                      flags.data_ptr(), stream), 4 * nf * 3, 2,
                     "stand-alone ema_kernel over the arena; includes the count launch"),
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
    assert float(flags[3]) == 0 and bool(torch.isfinite(arena.data).all())
    for name, (_, nbytes, per_call, note) in arms.items():
        v = sorted(ms[name])
        med = v[len(v) // 2]
        emit({"kind": "optimizer_kernel", "arm": name, "dtype": args.dtype, "params": n, "bytes": nbytes,
              "pack_bytes": pack_bytes if not name.endswith("_flat") else 0, "calls": args.rounds * args.launches,
              "device_launches_per_call": per_call, "us_median": round(med * 1e3, 2),
              "us_min": round(v[0] * 1e3, 2), "us_max": round(v[-1] * 1e3, 2),
              "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3), "note": note}, args.out)


def whole_step(args):
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    dev = torch.device("cuda", 0)
    for batch in (8, 1):
        img, gt = make_synthetic_batch(batch, 768, 1024, seed=0, device=dev)
        st = {}
        for name, lr, ema in (("sgd", 1e-7, 0.0), ("adam", 1e-5, 0.0), ("sgd_ema", 1e-7, 0.999),
                              ("adam_ema", 1e-5, 0.999)):
            torch.manual_seed(0)
            st[name] = NativeStepper(dev, dtype=args.dtype, lr=lr, batch=batch, graph=False,
                                     optimizer=name.split("_")[0], ema_decay=ema)
            for _ in range(args.warmup):
                st[name].step(img, gt)
        torch.cuda.synchronize()
        ips = {k: [] for k in st}
        for _ in range(args.rounds):
            for name, s in st.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    s.step(img, gt)
                torch.cuda.synchronize()
                ips[name].append(batch * args.steps / (time.perf_counter() - t0))
        for name, v in ips.items():
            v = sorted(v)
            emit({"kind": "whole_step", "optimizer": name, "dtype": args.dtype, "batch": batch, "size": "768x1024",
                  "graph": False, "steps": args.rounds * args.steps, "img_per_s_median": round(v[len(v) // 2], 2),
                  "img_per_s_min": round(v[0], 2), "img_per_s_max": round(v[-1], 2),
                  "finite": not st[name].nonfinite()}, args.out)
        del st


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=25, help="kernel arms: launches per arm and round")
    ap.add_argument("--steps", type=int, default=20, help="--whole-step: steps per arm and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--whole-step", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    (whole_step if args.whole_step else kernel_arms)(args)


if __name__ == "__main__":
    main()
