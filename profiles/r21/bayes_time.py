"""Device time of the Bayesian loss's launches at 8 x 48 x 64 cells (384 x 512 crops), 200 and 3000 heads per sample,
beside head_train's at the same shape in the same process: arms interleaved over rounds, device events around ITERS
back-to-back launches of one arm.  One JSON line per (heads, arm): the median over rounds and the spread.
Usage: python profiles/r21/bayes_time.py > bayes_time.jsonl"""
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from can_distributed_pytorch_amd.ops import _ext                      # noqa: E402
from can_distributed_pytorch_amd.ops.bayes import crop_points, _launch_loss   # noqa: E402

N, H, W, CH, CW, ITERS, ROUNDS = 8, 48, 64, 384, 512, 50, 7
C, st = _ext.require(), _ext.stream_ptr()
dev = "cuda"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS        # microseconds per call


for heads_per in (200, 3000):
    rng = np.random.default_rng(heads_per)
    # one image of 768 x 1024 per sample, its window the 384 x 512 in the middle: about a quarter of the records survive,
    # so the table holds 4 x heads_per records per sample
    tab = 4 * heads_per
    heads = np.stack([rng.integers(0, 1024, N * tab), rng.integers(0, 768, N * tab), np.full(N * tab, 2),
                      np.full(N * tab, 8)], 1).astype(np.float32)
    ranges = torch.tensor([[i * tab, tab] for i in range(N)], dtype=torch.int64)
    desc = torch.tensor([[0, 768, 1024, 3, i % 2, 192, 256, 1] for i in range(N)], dtype=torch.int64)
    hd, rd, dd = torch.from_numpy(heads).to(dev), ranges.to(dev), desc.to(dev)
    counts = [tab] * N
    target = crop_points(hd, rd, dd, N, CH, CW, counts=counts)
    et = (torch.rand(N, H, W, device=dev) + 0.5) * heads_per / (H * W)
    g = torch.empty(N, 1, H, W, device=dev)
    flags = torch.zeros(4, device=dev)
    scratch = (torch.empty(N, H, W, device=dev), torch.empty(N, H, W, device=dev))
    b6 = torch.randn(N, H, W, 64, device=dev).to(torch.bfloat16)
    w, b, gt = torch.randn(64, device=dev), torch.randn(1, device=dev), torch.rand(N, H, W, device=dev)
    P = N * H * W
    nblk = max(1, min(1024, (P * 8 + 255) // 256))
    part, dw, db, etb, dy = (torch.empty(s, device=dev) for s in (nblk * 66 + 1, 64, 1, P, 1))
    dy = torch.empty_like(b6)
    begins = target.begins

    def passes(mask):
        return lambda: _launch_loss(C, et, target, 8.0, 0.15, g, W, flags.data_ptr() + 4, flags.data_ptr(), mask, scratch)
    arms = {
        "crop_points": lambda: C.crop_points(hd.data_ptr(), rd.data_ptr(), dd.data_ptr(), begins.data_ptr(), N,
                                             target.pts.data_ptr(), target.cnt.data_ptr(), CH, CW, 8, st),
        "normaliser": passes(1), "expectation": passes(2), "gradient+loss": passes(4),
        "head_bwd": lambda: C.head_bwd(b6.data_ptr(), w.data_ptr(), g.data_ptr(), dy.data_ptr(), part.data_ptr(), nblk,
                                       dw.data_ptr(), db.data_ptr(), part.data_ptr() + 4 * nblk * 66, P, 1.0, 0.0, 0,
                                       0, st),
        "head_train": lambda: C.head_train(b6.data_ptr(), w.data_ptr(), b.data_ptr(), gt.data_ptr(), etb.data_ptr(),
                                           dy.data_ptr(), part.data_ptr(), nblk, dw.data_ptr(), db.data_ptr(),
                                           flags.data_ptr() + 4, P, 1.0, 0.0, 0, flags.data_ptr(), 0, st),
    }
    passes(7)()                                   # a finished run: every pass finds its inputs
    for fn in arms.values():
        timed(fn)                                 # warm-up
    res = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            res[k].append(timed(fn))
    kept = int(target.cnt.sum())
    for k, v in res.items():
        print(json.dumps(dict(cells=[N, H, W], heads_per_sample=kept / N, table_per_sample=tab, arm=k,
                              us_median=round(statistics.median(v), 2), us_min=round(min(v), 2),
                              us_max=round(max(v), 2), iters=ITERS, rounds=ROUNDS)), flush=True)
