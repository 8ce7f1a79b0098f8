"""Python front-end of the NHWC resampling kernels (csrc/resample.hip): adaptive average pool and bilinear resize.

x is an NHWC bf16 / fp16 map [N,H,W,C], contiguous, C % 8 == 0; the output [N,oh,ow,C] has x's dtype.  Shape / dtype /
layout checks are done here, before anything is launched.  The bilinear taps are formed here in float64 and uploaded
as one int32 table per axis, cached per (source length, output length, align_corners, device):

  i0[L], i1[L], lambda[L] (fp32 bits)      src = o (l - 1) / (L - 1) (align_corners; 0 when L == 1) or
                                           max(0, (o + 0.5) l / L - 0.5); i0 = floor(src), i1 = min(i0 + 1, l - 1),
                                           lambda = fp32(src - i0)
  w0[L], w1[L] (fp32 bits)                 the adjoint's weights on i0 / i1: fp32(1 - lambda) and lambda, or 1 and 0
                                           where i0 == i1 (the forward's fma(lambda, b - a, a) is a there)
  lo[l], hi[l]                             the outputs touching source s are exactly [lo[s], hi[s]) (monotone taps)
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from . import _ext
from .conv import MAX_ELEMS_PER_LAUNCH, _check_act, dt_code

POOL_FORMS = {"auto": 0, "direct": 1, "separable": 2}
_TABLES: Dict[Tuple[int, int, bool, str], torch.Tensor] = {}


def tap_table(l: int, L: int, align_corners: bool) -> np.ndarray:
    """The int32 table [5 L + 2 l] of one axis (module docstring), on the host."""
    o = np.arange(L, dtype=np.float64)
    if align_corners:
        src = o * (l - 1) / (L - 1) if L > 1 else np.zeros(L)
    else:
        src = np.maximum(0.0, (o + 0.5) * l / L - 0.5)
    i0 = np.minimum(np.floor(src).astype(np.int64), l - 1)
    i1 = np.minimum(i0 + 1, l - 1)
    lam = (src - i0).astype(np.float32)
    same = i0 == i1
    w0 = np.where(same, 1.0, 1.0 - lam.astype(np.float64)).astype(np.float32)
    w1 = np.where(same, np.float32(0), lam).astype(np.float32)
    s = np.arange(l)
    lo, hi = np.searchsorted(i1, s, side="left"), np.searchsorted(i0, s, side="right")
    return np.concatenate([i0.astype(np.int32), i1.astype(np.int32), lam.view(np.int32), w0.view(np.int32),
                           w1.view(np.int32), lo.astype(np.int32), hi.astype(np.int32)])


def _table(l: int, L: int, align_corners: bool, device: torch.device) -> torch.Tensor:
    key = (l, L, bool(align_corners), str(device))
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = torch.from_numpy(tap_table(l, L, align_corners)).to(device)
    return t


def _check(x: torch.Tensor, name: str, oh: int, ow: int) -> Tuple[int, int, int, int]:
    if x.dim() != 4:
        raise ValueError(f"{name} must be NHWC [N,H,W,C]")
    _check_act(x, name)
    n, h, w, c = x.shape
    if c == 0 or c % 8:
        raise ValueError(f"resampling needs C % 8 == 0, got {c}")
    if min(n, h, w, oh, ow) < 1:
        raise ValueError(f"every size must be >= 1, got {tuple(x.shape)} -> ({oh}, {ow})")
    if max(x.numel(), n * oh * ow * c) > MAX_ELEMS_PER_LAUNCH:
        raise ValueError(f"a map of more than {MAX_ELEMS_PER_LAUNCH} elements is too large for one launch")
    return n, h, w, c


def pool_plan(x_shape, oh: int, ow: int, form: str = "auto") -> dict:
    """{form: 1 direct / 2 separable, ws_floats} for a map of x_shape (resample_plan.h pool_plan)."""
    n, h, w, c = x_shape
    return _ext.require().pool_adaptive_plan(n, h, w, c, oh, ow, POOL_FORMS[form])


def adaptive_avg_pool(x: torch.Tensor, oh: int, ow: int, form: str = "auto") -> torch.Tensor:
    """F.adaptive_avg_pool2d: y[n,i,j] = fp32 sum of bin (i, j) / float(count), rounded once to x.dtype.
    form: "auto" (planned for the device), "direct" or "separable"."""
    n, h, w, c = _check(x, "x", oh, ow)
    C = _ext.require()
    p = C.pool_adaptive_plan(n, h, w, c, oh, ow, POOL_FORMS[form])
    ws = torch.empty(p["ws_floats"], dtype=torch.float32, device=x.device) if p["ws_floats"] else None
    y = torch.empty(n, oh, ow, c, dtype=x.dtype, device=x.device)
    C.pool_adaptive_fwd(x.data_ptr(), y.data_ptr(), ws.data_ptr() if ws is not None else 0, p["ws_floats"], n, h, w, c,
                        oh, ow, p["form"], dt_code(x.dtype), _ext.stream_ptr(x.device))
    return y


def adaptive_avg_pool_backward(dy: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """dx [N,h,w,C] of adaptive_avg_pool from dy [N,oh,ow,C]: a gather over the bins that hold each pixel."""
    n, oh, ow, c = _check(dy, "dy", h, w)
    dx = torch.empty(n, h, w, c, dtype=dy.dtype, device=dy.device)
    _ext.require().pool_adaptive_bwd(dy.data_ptr(), dx.data_ptr(), n, h, w, c, oh, ow, dt_code(dy.dtype),
                                     _ext.stream_ptr(dy.device))
    return dx


def resize_plan(x_shape, oh: int, ow: int, staged: int = -1, slices: int = 0) -> dict:
    """{fwd: {...}, bwd: {...}}: the forward and backward plans for a map of x_shape (resample_plan.h)."""
    n, h, w, c = x_shape
    C = _ext.require()
    return {"fwd": C.resize_bilinear_fwd_plan(n, h, w, c, oh, ow, staged),
            "bwd": C.resize_bilinear_bwd_plan(n, h, w, c, oh, ow, slices)}


def resize_bilinear(x: torch.Tensor, oh: int, ow: int, align_corners: bool = False, staged: int = -1) -> torch.Tensor:
    """F.interpolate(x, (oh, ow), mode="bilinear", align_corners=...): horizontal blend, then vertical, each
    fma(lambda, b - a, a) in fp32, rounded once to x.dtype.  staged: -1 planned, 1 LDS staging, 0 global reads."""
    n, h, w, c = _check(x, "x", oh, ow)
    if staged not in (-1, 0, 1):
        raise ValueError(f"staged={staged} must be -1 (planned), 0 or 1")
    tv, th = _table(h, oh, align_corners, x.device), _table(w, ow, align_corners, x.device)
    y = torch.empty(n, oh, ow, c, dtype=x.dtype, device=x.device)
    _ext.require().resize_bilinear_fwd(x.data_ptr(), y.data_ptr(), tv.data_ptr(), th.data_ptr(), n, h, w, c, oh, ow,
                                       staged, dt_code(x.dtype), _ext.stream_ptr(x.device))
    return y


def resize_bilinear_backward(dy: torch.Tensor, h: int, w: int, align_corners: bool = False,
                             slices: int = 0) -> torch.Tensor:
    """dx [N,h,w,C] of resize_bilinear from dy [N,oh,ow,C]: the exact adjoint as a gather.  slices: slices of each
    source row's output rows (0: planned for the device, 1 .. 64)."""
    n, oh, ow, c = _check(dy, "dy", h, w)
    if not 0 <= slices <= 64:
        raise ValueError(f"slices={slices} must be 0 (planned) or 1 .. 64")
    C = _ext.require()
    p = C.resize_bilinear_bwd_plan(n, h, w, c, oh, ow, slices)
    ws = torch.empty(p["ws_floats"], dtype=torch.float32, device=dy.device) if p["ws_floats"] else None
    tv, th = _table(h, oh, align_corners, dy.device), _table(w, ow, align_corners, dy.device)
    dx = torch.empty(n, h, w, c, dtype=dy.dtype, device=dy.device)
    C.resize_bilinear_bwd(dy.data_ptr(), dx.data_ptr(), tv.data_ptr(), th.data_ptr(),
                          ws.data_ptr() if ws is not None else 0, p["ws_floats"], n, h, w, c, oh, ow, p["S"],
                          dt_code(dy.dtype), _ext.stream_ptr(dy.device))
    return dx
