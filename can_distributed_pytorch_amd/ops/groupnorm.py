"""Python front-end of the NHWC group / instance normalisation kernels (csrc/groupnorm.hip).

F.group_norm(x, groups, weight, bias, eps) (+ ReLU) on an NHWC bf16 / fp16 map [N,H,W,C], C % 8 == 0, C % groups == 0,
fp32 affine parameters; statistics per (sample, group): stats fp32 [N, groups, 3] = (mean, biased var, rstd).
groups == C is instance norm.  Two forms (csrc/groupnorm_plan.h): "streamed" (statistics -> finalize -> apply, any size)
and "resident" (one kernel per direction, a sample's tile stays in LDS), planned per shape or forced.  Shape / dtype /
layout checks are done here, before anything is launched.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _ext
from .batchnorm import _vec
from .conv import _check_act, dt_code

AUTO, STREAMED, RESIDENT = 0, 1, 2
MAX_SLICES = 65535


def _check(x: torch.Tensor, groups: int, form: int, slices: int) -> Tuple[int, int, int, int]:
    if x.dim() != 4:
        raise ValueError("x must be NHWC [N,H,W,C]")
    _check_act(x, "x")
    n, h, w, c = x.shape
    if c == 0 or c % 8:
        raise ValueError(f"group norm needs C % 8 == 0, got {c}")
    if groups < 1 or c % groups:
        raise ValueError(f"groups={groups} must divide C={c}")
    if h * w * (c // groups) < 2:
        raise ValueError("group norm needs more than one value per (sample, group)")
    if n < 1 or n > MAX_SLICES or x.numel() > 1 << 48:
        raise ValueError(f"a map of {n} samples / {x.numel()} elements is beyond the kernels' indexing")
    if form not in (AUTO, STREAMED, RESIDENT):
        raise ValueError(f"form={form} must be 0 (planned), 1 (streamed) or 2 (resident)")
    if slices < 0 or slices > MAX_SLICES:
        raise ValueError(f"slices={slices} must be 0 (planned) or 1 .. {MAX_SLICES}")
    return n, h, w, c


def plan(x_shape, groups: int, backward: bool = False, form: int = AUTO, slices: int = 0) -> dict:
    """{form, S, bundle, spans, lds} for a map of x_shape (groupnorm_plan.h gn_plan); bundle = 0: the resident form
    cannot serve the shape (its tiles do not fit the LDS)."""
    n, h, w, c = x_shape
    return _ext.require().gn_plan(n, h, w, c, groups, int(backward), form, slices)


def _plan(x: torch.Tensor, groups: int, backward: bool, form: int, slices: int) -> dict:
    if form == RESIDENT and not plan(x.shape, groups, backward)["bundle"]:
        raise ValueError(f"the resident form cannot serve {tuple(x.shape)} with {groups} groups"
                         f"{' backward' if backward else ''}: its tiles do not fit the LDS")
    return plan(x.shape, groups, backward, form, slices)


def gn_forward(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, groups: int, eps: float, relu: bool,
               form: int = AUTO, slices: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, stats): y = [relu](group_norm(x)) in x.dtype, stats fp32 [N, groups, 3] = (mean, biased var, rstd).
    form: 0 planned, 1 streamed, 2 resident; slices: pixel slices of the streamed statistics pass (0: planned)."""
    C = _ext.require()
    n, h, w, c = _check(x, groups, form, slices)
    if not (eps >= 0.0) or eps == float("inf"):
        raise ValueError(f"eps={eps} must be finite and >= 0")
    wt, b = _vec(weight, c, "weight"), _vec(bias, c, "bias")
    p = _plan(x, groups, False, form, slices)
    part = ab = None
    if p["form"] == STREAMED:
        part = torch.empty(n, p["S"], 2, c, dtype=torch.float64, device=x.device)
        ab = torch.empty(n, 2, c, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    stats = torch.empty(n, groups, 3, dtype=torch.float32, device=x.device)
    C.gn_forward(x.data_ptr(), y.data_ptr(), wt.data_ptr(), b.data_ptr(), part.data_ptr() if part is not None else 0,
                 ab.data_ptr() if ab is not None else 0, stats.data_ptr(), n, h, w, c, groups, float(eps), int(relu),
                 dt_code(x.dtype), p["form"], p["S"], _ext.stream_ptr(x.device))
    return y, stats


def gn_backward(dy: torch.Tensor, x: torch.Tensor, y: torch.Tensor, weight: torch.Tensor, stats: torch.Tensor,
                groups: int, relu: bool, form: int = AUTO,
                slices: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dgamma, dbeta) of gn_forward from its input x, its output y (the ReLU mask is y > 0 on the stored 16-bit
    values; y is not read without relu) and its stats."""
    C = _ext.require()
    n, h, w, c = _check(x, groups, form, slices)
    _check_act(dy, "dy", dtype=x.dtype)
    if dy.shape != x.shape:
        raise ValueError("dy / x must be NHWC maps of one shape")
    if relu:
        _check_act(y, "y", dtype=x.dtype)
        if y.shape != x.shape:
            raise ValueError("y must have x's shape")
    if stats.dtype != torch.float32 or tuple(stats.shape) != (n, groups, 3) or not stats.is_cuda or \
            not stats.is_contiguous():
        raise ValueError(f"stats must be the forward's contiguous fp32 [{n}, {groups}, 3] tensor")
    wt = _vec(weight, c, "weight")
    p = _plan(x, groups, True, form, slices)
    part = torch.empty(n, p["S"], 2, c, dtype=torch.float64, device=x.device)
    c12 = torch.empty(n, groups, 2, dtype=torch.float32, device=x.device) if p["form"] == STREAMED else None
    dgb = torch.empty(2, c, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    C.gn_backward(dy.data_ptr(), x.data_ptr(), y.data_ptr() if relu else 0, wt.data_ptr(), stats.data_ptr(),
                  part.data_ptr(), c12.data_ptr() if c12 is not None else 0, dgb.data_ptr(), dx.data_ptr(), n, h, w, c,
                  groups, int(relu), dt_code(x.dtype), p["form"], p["S"], _ext.stream_ptr(x.device))
    return dx, dgb[0], dgb[1]
