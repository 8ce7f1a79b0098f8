"""usage: resize_time.py ARM_ROOT ARM_NAME ROUND -- GPU time of the resize launch (C.preprocess_batch) of the package
under ARM_ROOT, measured the way scripts/prof/crop_launch_time.py does: batch x HxW NHWC4 from packed uint8 RGB images
of the same size already on the device, hipEvents around 100 back-to-back launches, best and median of 7.  Also the
crop and scaled-crop launches at 8 x 384x512 bf16.  One JSON line per arm and shape."""
import json
import os
import sys

ARM, NAME, ROUND = os.path.abspath(sys.argv[1]), sys.argv[2], int(sys.argv[3])
sys.path.insert(0, ARM)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import can_distributed_pytorch_amd as pkg  # noqa: E402
assert os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__))) == ARM, pkg.__file__
from can_distributed_pytorch_amd.ops import _ext  # noqa: E402
from can_distributed_pytorch_amd.ops.conv import dt_code  # noqa: E402
from can_distributed_pytorch_amd.ops.preprocess import PackedCollate  # noqa: E402

C = _ext.require()
dev = torch.device("cuda")
st = _ext.stream_ptr(dev)
ITERS, REPS = 100, 7


def timed(launch):
    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            launch()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return round(min(us), 2), round(float(np.median(us)), 2)


rng = np.random.default_rng(0)
for batch, h, w in [(8, 384, 512), (1, 768, 1024), (8, 768, 1024)]:
    gt1 = torch.zeros(1, h // 8, w // 8)
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(batch)]
    packs = {"resize": PackedCollate()([(im, gt1, i % 2) for i, im in enumerate(imgs)])}
    if (batch, h) == (8, 384):
        packs["crop"] = PackedCollate(crop=(h, w))([(im, gt1[None], torch.tensor([[0, 0, i % 2]]))
                                                    for i, im in enumerate(imgs)])
        packs["crop_scaled"] = PackedCollate(crop=(h, w), crop_scale=True)(
            [(im, gt1[None], torch.tensor([[3, 5, i % 2, h - 40, w - 50]])) for i, im in enumerate(imgs)])
    for kind, (buf, meta) in packs.items():
        n, ho, wo, goff, doff = meta[:5]
        d = buf.to(dev)
        desc = d[doff:].view(torch.int64)
        for dtype in ((torch.bfloat16, torch.float16) if kind == "resize" else (torch.bfloat16,)):
            x4 = torch.empty(batch, h, w, 4, dtype=dtype, device=dev)
            dt = dt_code(dtype)
            if kind == "resize":
                def launch():
                    C.preprocess_batch(d.data_ptr(), 0, desc.data_ptr(), n, x4.data_ptr(), 0, ho, wo, 8, dt, st)
            else:
                fn = getattr(C, "preprocess_" + kind)

                def launch():
                    fn(d.data_ptr(), goff, desc.data_ptr(), buf.data_ptr() + doff, n, x4.data_ptr(), ho, wo, 8, dt, st)
            best, med = timed(launch)
            print(json.dumps(dict(arm=NAME, round=ROUND, launch=kind, batch=batch, out=[h, w],
                                  dtype=str(dtype).split(".")[1], us_best=best, us_median=med)), flush=True)
