"""5x5 / 7x7 convolutions, bf16, 8 images, forward / data gradient / weight gradient: the native NHWC kernels
(ops/conv.py conv_small / conv_small_wgrad with ksize 5 / 7, csrc/conv_large.hip) next to stock F.conv2d and
aten::convolution_backward on a channels_last tensor.  Arms interleaved in one process: 3 warm-up calls per arm, then
5 rounds of 10 calls each between device events; weight packs are built outside the timed region in both arms.

  python scripts/bench_conv_large.py [FILE]
"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from can_distributed_pytorch_amd.ops import conv as C  # noqa: E402

DEV = "cuda"
SHAPES = [(16, 32, 7, 1, 384, 512), (32, 32, 5, 1, 384, 512), (48, 48, 5, 2, 192, 256), (64, 64, 7, 1, 96, 128)]
N, ROUNDS, CALLS, WARM = 8, 5, 10, 3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / CALLS


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    print("layer | map | pass | native us (min..max) | stock us (min..max) | stock/native (medians)", file=out)
    for ci, co, k, dil, h, w in SHAPES:
        torch.manual_seed(0)
        pad = dil * (k // 2)
        x = torch.randn(N, h, w, ci, device=DEV).to(torch.bfloat16)
        dy = torch.randn(N, h, w, co, device=DEV).to(torch.bfloat16)
        wt = torch.randn(co, ci, k, k, device=DEV) * 0.05
        bias = torch.randn(co, device=DEV)
        wf, wd = C.pack_weight_fwd(wt, torch.bfloat16), C.pack_weight_dgrad(wt, torch.bfloat16)
        dw, db = torch.empty_like(wt), torch.empty_like(bias)
        ws = C.WgradWorkspace(x.device)
        y = torch.empty(N, h, w, co, device=DEV, dtype=torch.bfloat16)
        dx = torch.empty_like(x)
        # stock: NCHW-shaped views of the same NHWC memory = channels_last tensors
        xs, dys = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
        w16 = wt.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        b16 = bias.to(torch.bfloat16)
        cb = torch.ops.aten.convolution_backward
        geo = ([co], [1, 1], [pad, pad], [dil, dil], False, [0, 0], 1)
        arms = {
            "fwd": (lambda: C.conv_small(x, wf, bias, ksize=k, dil=dil, epi=C.EPI_BIAS, out=y),
                    lambda: F.conv2d(xs, w16, b16, padding=pad, dilation=dil)),
            "dgrad": (lambda: C.conv_small(dy, wd, None, ksize=k, dil=dil, epi=C.EPI_NONE, out=dx),
                      lambda: cb(dys, xs, w16, *geo, [True, False, False])),
            "wgrad": (lambda: C.conv_small_wgrad(dy, x, dw, db, ksize=k, dil=dil, ws=ws),
                      lambda: cb(dys, xs, w16, *geo, [False, True, True])),
        }
        # the two arms compute the same thing
        ref = F.conv2d(xs, w16, b16, padding=pad, dilation=dil).permute(0, 2, 3, 1).float()
        got = arms["fwd"][0]().float()
        rel = ((got - ref).norm() / ref.norm()).item()
        for name, (native, stock) in arms.items():
            for _ in range(WARM):
                native()
                stock()
            torch.cuda.synchronize()
            tn, ts = [], []
            for _ in range(ROUNDS):
                tn.append(timed(native))
                ts.append(timed(stock))
            print(f"{ci}->{co}k{k}d{dil} | {N}x{h}x{w} | {name} | {min(tn):.1f}..{max(tn):.1f} | "
                  f"{min(ts):.1f}..{max(ts):.1f} | {statistics.median(ts) / statistics.median(tn):.2f}x"
                  + (f" | fwd rel diff {rel:.1e}" if name == "fwd" else ""), file=out, flush=True)


if __name__ == "__main__":
    main()
