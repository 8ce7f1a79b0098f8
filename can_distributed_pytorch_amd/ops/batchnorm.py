"""Python front-end of the NHWC batch-normalisation kernels (csrc/batchnorm.hip).

nn.BatchNorm2d (+ ReLU) on an NHWC bf16 / fp16 map [N,H,W,C], C % 8 == 0, fp32 affine parameters and statistics:
the reference's ``make_layers(batch_norm=True)`` layer (model/CANNet.py:116-117) between a conv and the pool.  The
statistics need the whole batch, so there is no image chunking: one launch set addresses the map with 64-bit pixel
offsets.  Shape / dtype / layout checks are done here, before anything is launched.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _ext
from .conv import _check_act, dt_code


def _vec(t: Optional[torch.Tensor], c: int, name: str) -> torch.Tensor:
    if t is None or t.dtype != torch.float32 or t.numel() != c or not t.is_cuda:
        raise ValueError(f"{name} must be an fp32 GPU tensor [{c}]")
    t = t.detach().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()      # the kernels read the vectors in 16-byte pieces


def _workspace(x: torch.Tensor, slices: int) -> Tuple[torch.Tensor, int]:
    """The double partials [S, 2, C] of one statistics pass; slices = 0: the planned count."""
    m, c = x.numel() // x.shape[-1], x.shape[-1]
    if slices < 0 or slices > 65535:
        raise ValueError(f"slices={slices} must be 0 (planned) or 1 .. 65535")
    s = slices or _ext.require().bn_slices(m, c)
    return torch.empty(s, 2, c, dtype=torch.float64, device=x.device), s


def bn_forward(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, running_mean: Optional[torch.Tensor],
               running_var: Optional[torch.Tensor], training: bool, eps: float, relu: bool,
               slices: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, stats): y = [relu](batch_norm(x)) in x.dtype, stats fp32 [3, C] = (mean, biased var, rstd) of the batch
    (training) or (running_mean, running_var, 1 / sqrt(running_var + eps)) (eval).  The running buffers are read in
    eval mode only and never written.  slices: pixel slices of the statistics pass (0: planned for the device)."""
    C = _ext.require()
    if x.dim() != 4:
        raise ValueError("x must be NHWC [N,H,W,C]")
    _check_act(x, "x")
    c = x.shape[-1]
    m = x.numel() // max(c, 1)
    if c == 0 or c % 8:
        raise ValueError(f"batch norm needs C % 8 == 0, got {c}")
    if training and m < 2:
        raise ValueError("training batch norm needs more than one value per channel")
    if not (eps >= 0.0) or eps == float("inf"):
        raise ValueError(f"eps={eps} must be finite and >= 0")
    w, b = _vec(weight, c, "weight"), _vec(bias, c, "bias")
    rm = rv = None
    part, s = None, 0
    if training:
        part, s = _workspace(x, slices)
    else:
        rm, rv = _vec(running_mean, c, "running_mean"), _vec(running_var, c, "running_var")
    y = torch.empty_like(x)
    stats = torch.empty(3, c, dtype=torch.float32, device=x.device)
    ab = torch.empty(2, c, dtype=torch.float32, device=x.device)
    C.bn_forward(x.data_ptr(), y.data_ptr(), w.data_ptr(), b.data_ptr(), rm.data_ptr() if rm is not None else 0,
                 rv.data_ptr() if rv is not None else 0, part.data_ptr() if part is not None else 0, s,
                 stats.data_ptr(), ab.data_ptr(), m, c, float(eps), int(training), int(relu), dt_code(x.dtype),
                 _ext.stream_ptr(x.device))
    return y, stats


def bn_backward(dy: torch.Tensor, x: torch.Tensor, y: torch.Tensor, weight: torch.Tensor, stats: torch.Tensor,
                training: bool, relu: bool, slices: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dgamma, dbeta) of bn_forward from its input x, its output y (the ReLU mask is y > 0 on the stored 16-bit
    values; y is not read without relu) and its stats.  Eval: dx = weight * rstd * dz; dgamma / dbeta as in training."""
    C = _ext.require()
    _check_act(x, "x")
    _check_act(dy, "dy", dtype=x.dtype)
    if x.dim() != 4 or dy.shape != x.shape:
        raise ValueError("dy / x must be NHWC maps of one shape")
    c = x.shape[-1]
    m = x.numel() // max(c, 1)
    if c == 0 or c % 8:
        raise ValueError(f"batch norm needs C % 8 == 0, got {c}")
    if relu:
        _check_act(y, "y", dtype=x.dtype)
        if y.shape != x.shape:
            raise ValueError("y must have x's shape")
    if stats.dtype != torch.float32 or tuple(stats.shape) != (3, c) or not stats.is_cuda or \
            not stats.is_contiguous() or stats.data_ptr() % 16:
        raise ValueError(f"stats must be the forward's contiguous fp32 [3, {c}] tensor")
    w = _vec(weight, c, "weight")
    part, s = _workspace(x, slices)
    fin = torch.empty(4, c, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    C.bn_backward(dy.data_ptr(), x.data_ptr(), y.data_ptr() if relu else 0, w.data_ptr(), stats.data_ptr(),
                  part.data_ptr(), s, fin.data_ptr(), dx.data_ptr(), m, c, int(training), int(relu),
                  dt_code(x.dtype), _ext.stream_ptr(x.device))
    return dx, fin[0], fin[1]
