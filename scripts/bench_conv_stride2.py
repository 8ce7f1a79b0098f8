"""Stride-2 down-sampling and 2x transposed convolutions, bf16, 8 images, forward / data gradient / weight gradient:
the native NHWC kernels (ops/conv.py conv_down2 / conv_up2 / conv_s2_wgrad, csrc/conv_stride2.hip) next to stock
F.conv2d(stride=2) / F.conv_transpose2d and aten::convolution_backward on channels_last tensors.  Arms interleaved in
one process: 3 warm-up calls per arm, then 5 rounds of 10 calls each between device events; weight packs are built
outside the timed region in both arms.  Map sizes name the LARGE map.

  python scripts/bench_conv_stride2.py [FILE]
"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from can_distributed_pytorch_amd.ops import conv as C  # noqa: E402

DEV = "cuda"
# kind, ci, co, k, large map (h, w)
SHAPES = [("down", 64, 128, 3, 384, 512), ("down", 256, 512, 1, 96, 128), ("up", 64, 64, 2, 192, 256),
          ("up", 128, 64, 4, 192, 256)]
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
    bf = torch.bfloat16
    print("layer | large map | pass | native us (min..max) | stock us (min..max) | stock/native (medians)", file=out)
    for kind, ci, co, k, h, w in SHAPES:
        torch.manual_seed(0)
        up, p = kind == "up", (k - 1) // 2
        cbig, csmall = (co, ci) if up else (ci, co)
        big = torch.randn(N, h, w, cbig, device=DEV).to(bf)             # down: x, up: dY
        small = torch.randn(N, h // 2, w // 2, csmall, device=DEV).to(bf)   # down: dY, up: x
        wt = torch.randn(*((ci, co) if up else (co, ci)), k, k, device=DEV) * 0.05
        bias = torch.randn(co, device=DEV)
        dw, db = torch.empty_like(wt), torch.empty_like(bias)
        ws = C.WgradWorkspace(big.device)
        obig, osmall = torch.empty_like(big), torch.empty_like(small)
        bs, ss = big.permute(0, 3, 1, 2), small.permute(0, 3, 1, 2)      # channels_last views of the same memory
        w16 = wt.to(bf).contiguous(memory_format=torch.channels_last)
        b16 = bias.to(bf)
        cb = torch.ops.aten.convolution_backward
        geo = ([co], [2, 2], [p, p], [1, 1], up, [k % 2, k % 2] if up else [0, 0], 1)
        if up:
            wf, wd = C.pack_weight_up(wt, bf), C.pack_weight_fwd(wt, bf)
            stock_fwd = lambda: F.conv_transpose2d(ss, w16, b16, stride=2, padding=p, output_padding=k % 2)  # noqa: E731
            arms = {
                "fwd": (lambda: C.conv_up2(small, wf, bias, ksize=k, epi=C.EPI_BIAS, out=obig), stock_fwd),
                "dgrad": (lambda: C.conv_down2(big, wd, None, ksize=k, epi=C.EPI_NONE, out=osmall),
                          lambda: cb(bs, ss, w16, *geo, [True, False, False])),
                "wgrad": (lambda: C.conv_s2_wgrad(small, big, dw, db, ksize=k, bias_of="big", ws=ws),
                          lambda: cb(bs, ss, w16, *geo, [False, True, True])),
            }
        else:
            wf, wd = C.pack_weight_fwd(wt, bf), C.pack_weight_up(wt, bf)
            stock_fwd = lambda: F.conv2d(bs, w16, b16, stride=2, padding=p)  # noqa: E731
            arms = {
                "fwd": (lambda: C.conv_down2(big, wf, bias, ksize=k, epi=C.EPI_BIAS, out=osmall), stock_fwd),
                "dgrad": (lambda: C.conv_up2(small, wd, None, ksize=k, epi=C.EPI_NONE, out=obig),
                          lambda: cb(ss, bs, w16, *geo, [True, False, False])),
                "wgrad": (lambda: C.conv_s2_wgrad(small, big, dw, db, ksize=k, bias_of="small", ws=ws),
                          lambda: cb(ss, bs, w16, *geo, [False, True, True])),
            }
        # the two arms compute the same thing
        ref = stock_fwd().permute(0, 2, 3, 1).float()
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
            ratio = statistics.median(ts) / statistics.median(tn)
            print(f"{kind} {ci}->{co}k{k} | {N}x{h}x{w} | {name} | {min(tn):.1f}..{max(tn):.1f} | "
                  f"{min(ts):.1f}..{max(ts):.1f} | {ratio:.2f}x" + (" TRAILS" if ratio < 1.0 else "")
                  + (f" | fwd rel diff {rel:.1e}" if name == "fwd" else ""), file=out, flush=True)


if __name__ == "__main__":
    main()
