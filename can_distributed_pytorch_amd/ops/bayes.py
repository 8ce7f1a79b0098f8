"""Bayesian point loss (Ma et al., ICCV 2019) on head records: csrc/bayes.hip (README, "Bayesian loss").

``crop_points`` turns the head table of a heads pack into the points of every crop (a ``PointTarget``);
``bayes_loss`` is the loss of a density map against such a target: the loss, its gradient with respect to the map and
the expected count of every head.  The native step reaches both through ``preprocess_packed(points=True)`` /
``AheadPrep(points=True)`` and ``CANNetExecutor.head_train_bayes``.  There is no route outside HIP.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _ext


class PointTarget:
    """The heads of n crops of (ch, cw) pixels as points, the target of a map [n, h, w].

    pts [T, 2] fp32 (x, y) in crop pixels; begins [n + 1] int64 (device), sample s owns the slots begins[s] ..
    begins[s + 1] of pts; cnt [n] int32 (device), the first cnt[s] of its slots hold its heads.  max_count, the
    largest number of slots of a sample, sizes a launch grid: given by whoever knows it on the host (the pack's ranges),
    else read back from begins once."""

    def __init__(self, pts, begins, cnt, n, h, w, ch, cw, max_count: Optional[int] = None):
        n, h, w, ch, cw = int(n), int(h), int(w), int(ch), int(cw)
        if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 2 or not pts.is_contiguous():
            raise ValueError("pts must be a contiguous fp32 [T, 2]")
        if begins.dtype != torch.int64 or tuple(begins.shape) != (n + 1,) or not begins.is_contiguous():
            raise ValueError(f"begins must be a contiguous int64 [{n + 1}]")
        if cnt.dtype != torch.int32 or tuple(cnt.shape) != (n,) or not cnt.is_contiguous():
            raise ValueError(f"cnt must be a contiguous int32 [{n}]")
        if n < 1 or h < 1 or w < 1 or ch % h or cw % w or ch // h != cw // w:
            raise ValueError(f"a map [{n}, {h}, {w}] is no downsampled crop of {ch} x {cw}")
        self.pts, self.begins, self.cnt = pts, begins, cnt
        self.n, self.h, self.w, self.ch, self.cw = n, h, w, ch, cw
        if max_count is None:
            max_count = int((begins[1:] - begins[:-1]).max().item())
        self.max_count = int(max_count)

    @property
    def shape(self):
        return ("points", self.n, self.h, self.w)

    @property
    def device(self):
        return self.pts.device

    def data_ptr(self):
        return self.pts.data_ptr()

    def tensors(self):
        return self.pts, self.begins, self.cnt

    def record_stream(self, stream):
        for t in self.tensors():
            t.record_stream(stream)

    def to(self, device, non_blocking: bool = False):
        if torch.device(device) == self.device:
            return self
        p, b, c = (t.to(device, non_blocking=non_blocking) for t in self.tensors())
        return PointTarget(p, b, c, self.n, self.h, self.w, self.ch, self.cw, self.max_count)


def crop_points(heads, ranges, desc, n, ch, cw, downsample: int = 8, counts=None, stream=None) -> PointTarget:
    """heads [*, 4] fp32 (c, r, ., .), ranges [n, 2] int64 (first head, head count) and desc [n, 8] int64 of a heads pack
    that passed gt_from_heads_check, all on the device -> the PointTarget of its n crops.  A record is kept iff its
    pixel lies in the sample's window; the survivors keep table order.  counts: the head counts on the host (the slots
    of every sample), else they are read back from ranges."""
    C = _ext.require()
    dev = heads.device
    if counts is None:
        counts = ranges[:, 1].tolist()
    total, mx = int(sum(counts)), int(max(counts))
    begins = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(ranges[:, 1], 0, out=begins[1:])
    pts = torch.empty(max(total, 1), 2, dtype=torch.float32, device=dev)[:total]
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    C.crop_points(heads.data_ptr(), ranges.data_ptr(), desc.data_ptr(), begins.data_ptr(), n, pts.data_ptr(),
                  cnt.data_ptr(), ch, cw, downsample, _ext.stream_ptr(dev) if stream is None else stream)
    return PointTarget(pts, begins, cnt, n, ch // downsample, cw // downsample, ch, cw, mx)


def _check_params(sigma, bg_ratio):
    if not sigma > 0:
        raise ValueError(f"sigma must be > 0, got {sigma!r}")
    if not 0 <= bg_ratio <= 1:
        raise ValueError(f"bg_ratio must be in [0, 1], got {bg_ratio!r}")


def _launch_loss(C, et, target: PointTarget, sigma, bg_ratio, g, gpitch, loss_ptr, nf_ptr, passes=7, scratch=None):
    """The three passes on et [n, h, w] (dense).  Returns (E, (lse, dmin)); g [n, h, gpitch] is written in place."""
    n, h, w = target.n, target.h, target.w
    T = target.pts.shape[0]
    dev = et.device
    lse, dmin = scratch if scratch is not None else (torch.empty(n, h, w, dtype=torch.float32, device=dev),
                                                      torch.empty(n, h, w, dtype=torch.float32, device=dev))
    E = torch.empty(T + n, dtype=torch.float32, device=dev)
    C.bayes_loss(et.data_ptr(), target.pts.data_ptr(), target.begins.data_ptr(), target.cnt.data_ptr(), n, h, w, T,
                 target.max_count, float(sigma), float(bg_ratio), target.ch, target.cw, target.ch // h,
                 lse.data_ptr(), dmin.data_ptr(), E.data_ptr(), g.data_ptr(), gpitch, loss_ptr, nf_ptr,
                 _ext.stream_ptr(dev), passes)
    return E, (lse, dmin)


def bayes_loss(et, target: PointTarget, sigma: float = 8.0, bg_ratio: float = 0.15):
    """et [n, h, w] or [n, 1, h, w] fp32 on the GPU -> (loss [1], g like et, E [T + n]).  E holds the expected count of
    every head in its slot of target.pts (0 in a slot without a head), then E_0 of every sample: the background's with
    bg_ratio > 0, the map's sum for a sample without heads, else 0."""
    C = _ext.require()
    _check_params(sigma, bg_ratio)
    n, h, w = target.n, target.h, target.w
    if et.dtype != torch.float32 or tuple(et.shape) not in ((n, h, w), (n, 1, h, w)) or not et.is_cuda:
        raise ValueError(f"et must be fp32 [{n}, {h}, {w}] or [{n}, 1, {h}, {w}] on the GPU, got {tuple(et.shape)} "
                         f"{et.dtype}")
    target = target.to(et.device)
    etc = et.contiguous()
    g = torch.empty_like(etc)
    loss = torch.empty(1, dtype=torch.float32, device=et.device)
    E, _ = _launch_loss(C, etc, target, sigma, bg_ratio, g, w, loss.data_ptr(), 0)
    return loss, g, E
