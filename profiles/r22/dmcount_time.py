"""Device time of the DM-Count loss at 8 x 48 x 64 cells (384 x 512 crops), about 200 and 3000 heads per sample.

  python profiles/r22/dmcount_time.py > dmcount_time.jsonl
      device events around ITERS back-to-back calls of the whole loss (2 T + 2 launches) with T = 100, 50 and 1, the
      arms interleaved over rounds; one JSON line per (heads, T): the median over rounds and the spread
  rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python profiles/r22/dmcount_time.py trace HEADS [tight]
      CALLS calls of the loss with T = 100 at HEADS heads per sample, for the per-kernel times of the trace's statistics
"""
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from can_distributed_pytorch_amd.ops import _ext                      # noqa: E402
from can_distributed_pytorch_amd.ops.bayes import crop_points         # noqa: E402
from can_distributed_pytorch_amd.ops.dmcount import _launch_loss, head_tile   # noqa: E402

N, H, W, CH, CW, ITERS, ROUNDS, CALLS = 8, 48, 64, 384, 512, 10, 7, 20
C = _ext.require()
dev = "cuda"


def setup(heads_per, tight=False):
    """One image of 768 x 1024 per sample, its window the 384 x 512 in the middle: about a quarter of the records
    survive, so the table holds 4 x heads_per records per sample and max_count, which sizes the grid and picks the
    head tile, is 4 x heads_per as in training.  tight: max_count = the most heads that survived in a sample."""
    rng = np.random.default_rng(heads_per)
    tab = 4 * heads_per
    heads = np.stack([rng.integers(0, 1024, N * tab), rng.integers(0, 768, N * tab), np.full(N * tab, 2),
                      np.full(N * tab, 8)], 1).astype(np.float32)
    ranges = torch.tensor([[i * tab, tab] for i in range(N)], dtype=torch.int64)
    desc = torch.tensor([[0, 768, 1024, 3, i % 2, 192, 256, 1] for i in range(N)], dtype=torch.int64)
    target = crop_points(torch.from_numpy(heads).to(dev), ranges.to(dev), desc.to(dev), N, CH, CW, counts=[tab] * N)
    if tight:
        target.max_count = int(target.cnt.max())
    et = (torch.rand(N, H, W, device=dev) + 0.5) * heads_per / (H * W)
    g = torch.empty(N, 1, H, W, device=dev)
    flags = torch.zeros(4, device=dev)
    return target, lambda T: _launch_loss(C, et, target, 10.0, T, 0.1, 0.01, g, W, flags.data_ptr() + 4,
                                          flags.data_ptr())


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS        # microseconds per call


if sys.argv[1:2] == ["trace"]:
    _, loss = setup(int(sys.argv[2]), sys.argv[3:4] == ["tight"])
    for _ in range(CALLS):
        loss(100)
    torch.cuda.synchronize()
    sys.exit(0)

for heads_per, tight in ((200, False), (200, True), (3000, False), (3000, True)):
    target, loss = setup(heads_per, tight)
    arms = {T: (lambda T=T: loss(T)) for T in (100, 50, 1)}
    for fn in arms.values():
        timed(fn)                                 # warm-up
    res = {T: [] for T in arms}
    for _ in range(ROUNDS):
        for T, fn in arms.items():
            res[T].append(timed(fn))
    for T, v in res.items():
        print(json.dumps(dict(cells=[N, H, W], heads_per_sample=int(target.cnt.sum()) / N, max_count=target.max_count,
                              tile=head_tile(target.max_count), sinkhorn_iters=T, launches=2 * T + 2,
                              us_median=round(statistics.median(v), 1), us_min=round(min(v), 1),
                              us_max=round(max(v), 1), calls=ITERS, rounds=ROUNDS)), flush=True)
