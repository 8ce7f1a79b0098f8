"""Masked counts and GAME metrics (README, "ROI masks and GAME").

A ground truth may travel with a per-pixel loss weight as one fp32 tensor [n, 2, h, w]: channel 0 the ground truth,
channel 1 the weight m (the ROI mask's exact area mean per cell, data/transforms.py:roi_weights).  A [n, 1, h, w]
tensor means "no weight".  ``split_gt`` makes the two views, ``weighted_sq_loss`` is the autograd steppers' loss and
``count_metrics`` the evaluation side:

  level-l cell (a, b) covers rows [(a h) >> l, ((a+1) h) >> l) and the columns likewise with w, l = 0..3;
  E_cell = sum double(m) double(et), G_cell the same with gt (every product exact);
  GAME_l = sum over the level's cells of |E_cell - G_cell|;   per sample float64 (E, G, GAME_0 .. GAME_3).

Every level's cells are unions of level-3 cells ((a h) >> l == (a 2^(3-l) h) >> 3), a map smaller than 8 has empty
cells that add 0, and GAME_0 = |E - G| is the sample's absolute count error.  On a GPU the two launches of
csrc/elementwise.hip (count_metrics_kernel, count_metrics_final_kernel: fixed-order double sums, no atomics,
bitwise repeatable) compute it; on the CPU the same definition in torch float64.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ..parallel.distributed import get_world_size, reduce_scalars

GAME_LEVELS = 4


def split_gt(gt: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(ground truth [n,1,h,w], weight [n,1,h,w] or None) views of a [n,1,h,w] or [n,2,h,w] ground-truth tensor."""
    if gt.dim() != 4 or gt.shape[1] not in (1, 2):
        raise ValueError(f"a ground truth is [n, 1, h, w], or [n, 2, h, w] with a loss weight, got {tuple(gt.shape)}")
    if gt.shape[1] == 1:
        return gt, None
    return gt[:, 0:1], gt[:, 1:2]


def weighted_sq_loss(et: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """MSELoss(sum) of et against a 1-channel gt (exactly torch's), ((et - gt)^2 m).sum() against a 2-channel one."""
    g, m = split_gt(gt)
    if m is None:
        return torch.nn.functional.mse_loss(et, g, reduction="sum")
    d = et - g
    return (d * d * m).sum()


def _cell_edges(size: int, level: int):
    return [(a * size) >> level for a in range((1 << level) + 1)]


def count_metrics_torch(et: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """The definition in torch float64 (any device): float64 [n, 6] = (E, G, GAME_0 .. GAME_3)."""
    g, m = split_gt(gt)
    if et.dim() != 4 or et.shape[1] != 1 or tuple(et.shape) != tuple(g.shape):
        raise ValueError(f"et {tuple(et.shape)} and gt {tuple(gt.shape)} must be [n, 1, h, w] and [n, 1 or 2, h, w]")
    e64, g64 = et.double(), g.double()
    if m is not None:
        e64, g64 = e64 * m.double(), g64 * m.double()
    n, _, h, w = e64.shape
    out = torch.zeros(n, 2 + GAME_LEVELS, dtype=torch.float64, device=et.device)
    ys, xs = _cell_edges(h, 3), _cell_edges(w, 3)
    # the 64 level-3 cell sums, then every level as sums of those
    ce = torch.stack([torch.stack([e64[:, 0, ys[a]:ys[a + 1], xs[b]:xs[b + 1]].sum(dim=(1, 2)) for b in range(8)], 1)
                      for a in range(8)], 1)
    cg = torch.stack([torch.stack([g64[:, 0, ys[a]:ys[a + 1], xs[b]:xs[b + 1]].sum(dim=(1, 2)) for b in range(8)], 1)
                      for a in range(8)], 1)
    for level in range(GAME_LEVELS):
        side, span = 1 << level, 8 >> level
        le = ce.reshape(n, side, span, side, span).sum(dim=(2, 4))
        lg = cg.reshape(n, side, span, side, span).sum(dim=(2, 4))
        out[:, 2 + level] = (le - lg).abs().sum(dim=(1, 2))
        if level == 0:
            out[:, 0], out[:, 1] = le[:, 0, 0], lg[:, 0, 0]
    return out


def count_metrics(et: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """float64 [n, 6] = (E, G, GAME_0 .. GAME_3) per sample of et [n,1,h,w] against gt [n,1,h,w] or, with a weight
    plane, [n,2,h,w].  GPU tensors go through the native kernels (the extension is required there: no fallback), CPU
    tensors through ``count_metrics_torch``.  No host sync either way."""
    if not et.is_cuda:
        return count_metrics_torch(et, gt)
    from ..ops import _ext
    C = _ext.require()
    g, m = split_gt(gt)
    if et.dim() != 4 or et.shape[1] != 1 or tuple(et.shape) != tuple(g.shape):
        raise ValueError(f"et {tuple(et.shape)} and gt {tuple(gt.shape)} must be [n, 1, h, w] and [n, 1 or 2, h, w]")
    if gt.device != et.device:
        raise ValueError("et and gt must be on the same device")
    et = et.float().contiguous()
    gt = gt.float().contiguous()
    n, _, h, w = et.shape
    part = torch.empty(n, 64, 2, dtype=torch.float64, device=et.device)
    out = torch.empty(n, 2 + GAME_LEVELS, dtype=torch.float64, device=et.device)
    stride = gt.shape[1] * h * w
    with torch.cuda.device(et.device):
        C.count_metrics(et.data_ptr(), gt.data_ptr(), stride, gt.data_ptr() + 4 * h * w if m is not None else 0, stride,
                        n, h, w, part.data_ptr(), out.data_ptr(), _ext.stream_ptr(et.device))
    return out


@torch.no_grad()
def evaluate_metrics(model, loader, device, prep=None):
    """Masked count metrics of ``model`` over ``loader``, summed: a dict of Python floats
    {"n", "game": [sum GAME_0 .. sum GAME_3], "se": sum (E - G)^2}, SUM-reduced over ranks by ONE collective.  The
    sums are kept on the device (no host sync per image); the caller divides: mae = game[0] / n, rmse = sqrt(se / n),
    game_l = game[l] / n.  ``prep`` maps a raw loader batch to (img, gt) on the device, gt 1- or 2-channel."""
    model.eval()
    acc = torch.zeros(2 + GAME_LEVELS, dtype=torch.float64, device=device)      # n, se, GAME_0..3
    for batch in loader:
        img, gt = prep(batch) if prep is not None else batch
        img, gt = img.to(device, non_blocking=True), gt.to(device, non_blocking=True)
        cm = count_metrics(model(img).float(), gt)
        d = cm[:, 0] - cm[:, 1]
        acc[0] += cm.shape[0]
        acc[1] += (d * d).sum()
        acc[2:] += cm[:, 2:].sum(dim=0)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    # one collective for all six sums (it carries fp32); a single process keeps its float64 sums
    vec = (reduce_scalars(*acc.unbind(0), average=False) if get_world_size() > 1 else acc).tolist()
    return {"n": int(round(vec[0])), "se": vec[1], "game": vec[2:]}
