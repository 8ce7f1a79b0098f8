"""`torch.ops.cannet.*`: the native gfx950 kernels as PyTorch custom operators (SURVEY §7.1 "host framework").

The CANNet executor (ops/executor.py) schedules the whole network itself.  These registrations expose the same
kernels to ANY model: each op has a real GPU implementation (the MFMA kernels), a fake (meta) implementation for
shape propagation — so ``torch.compile`` traces them without graph breaks and ``FakeTensorMode`` works without a
GPU — and an autograd formula built from the native backward kernels.

  cannet::conv2d_nhwc(x, weight, bias, dilation, relu) -> y
      x [N,H,W,Ci] bf16/fp16 (NHWC, contiguous), weight [Co,Ci,k,k] fp32 master (k = 1, 3, 5 or 7), bias [Co] fp32
      or None; stride 1, 'same' padding dilation*(k//2); y = [relu](conv(x, weight) + bias) in x.dtype.
      k = 5 (dilation 1 - 2) and k = 7 (dilation 1), the layers of multi-column and scale-aggregation networks, run
      on the streamed-weight kernels of csrc/conv_large.hip whatever the channel multiples (``conv_small`` /
      ``conv_small_wgrad`` with ksize 5 / 7); the rest of this entry is about k = 1 and 3.
      Ci, Co multiples of 16 (the first 3-channel layer has its own kernel inside the executor).  When both are
      multiples of 64 the op runs on the 64-channel-chunk kernels described next; otherwise (a 32-, 48- or 96-channel
      stage, a 1x1 bottleneck to 16 channels, a 160-channel trunk ...) forward, data gradient and weight gradient run
      on the small-channel MFMA kernels of csrc/conv_small.hip (``conv_small`` / ``conv_small_wgrad``: dilation 1..4,
      same packs, same epilogues, same deterministic slice reduction), with no padding to 64 channels.
      Forward: conv_igemm (bias + ReLU epilogue).  Backward: dY masked by y > 0, the data gradient on the same
      kernel with the flipped / transposed weight pack, the weight + bias gradients on the split-pixel weight-
      gradient kernels (fp32, deterministic slab reduction) — the reference's nn.Conv2d + ReLU
      (model/CANNet.py:14-17, 114-115) as one op.
  cannet::conv2d_thin_nhwc(x, weight, bias, dilation, relu, fp32_out) -> y
      the stem and the head of a network: conv2d_nhwc's contract for layers in which exactly one of Ci, Co is
      1 .. 8 (the real count: an RGB image is [N,H,W,3], 6 bytes per pixel) and the other a multiple of 16; k = 1
      or 3, dilation 1 .. 4.  fp32_out (thin Co only): y in fp32, for a density map that gets summed into a count.
      Runs on csrc/conv_thin.hip: few -> many (stem forward, head data gradient) and many -> few (head forward,
      stem data gradient) MFMA kernels, one weight-gradient kernel + deterministic slice reduce.  The data gradient
      is computed only when x requires one.
  cannet::conv2d_down2_nhwc(x, weight, bias, relu) -> y
      the learned down-sampling of a backbone: F.conv2d(x, weight, bias, stride=2, padding=(k - 1) // 2) [+ ReLU], x
      [N,H,W,Ci] with H and W even, weight [Co,Ci,k,k] fp32, k = 1 .. 4, Ci and Co any multiples of 16, y
      [N,H/2,W/2,Co].  Runs on csrc/conv_stride2.hip: a stride-2 gather out of a window staged split by column
      parity.  Backward: dY masked by y > 0, the data gradient as the transposed conv below (``conv_up2`` on
      ``pack_weight_up(weight)``), the weight + bias gradients on the stride-2 weight-gradient kernel
      (``conv_s2_wgrad``, deterministic slice reduction).
  cannet::conv_transpose2d_up2_nhwc(x, weight, bias, relu) -> y
      the learned 2x up-sampling of a decoder: F.conv_transpose2d(x, weight, bias, stride=2, padding=(k - 1) // 2,
      output_padding=k % 2) [+ ReLU], x [N,h,w,Ci], weight [Ci,Co,k,k] fp32 (nn.ConvTranspose2d's layout), k = 1 .. 4,
      y [N,2h,2w,Co].  Same unit: the four output parity classes as stride-1 convs of the small map over the taps
      that reach them, no scatter and no inserted zeros.  Backward: the data gradient is the down-sampling conv
      (``conv_down2`` on ``pack_weight_fwd(weight)``), the weight gradient the same kernel with the operands' roles
      swapped, which yields [Ci,Co,k,k] directly.
  cannet::relu_max_pool2x2(x) -> (y, codes)
      the ReLU-fused 2x2 / stride-2 max-pool of an NHWC map: y = max_pool2d(relu(x), 2) (= relu of the window
      max); codes = int32 first-max one-hots (4 bits per channel, 0 where the window max is <= 0).  Backward
      scatters through the codes, so the ReLU's mask is part of the gradient: exactly the gradient of
      max_pool2d(relu(x)), and of a plain max-pool only where the input is already non-negative.
  cannet::batch_norm_nhwc(x, weight, bias, running_mean, running_var, training, eps, relu) -> (y, stats)
      nn.BatchNorm2d [+ ReLU] of an NHWC bf16/fp16 map, C % 8 == 0, fp32 parameters (csrc/batchnorm.hip): training
      normalises with the batch statistics (double partial sums in a fixed order: bitwise repeatable), eval with
      (running_mean, running_var).  Functional: the running buffers are never written; stats = fp32 [3, C] (mean,
      biased variance, rstd), not differentiable, is what the backward and ``BatchNorm2dNHWC``'s buffer update use.
      Backward: dz = dY masked by the stored y > 0, then dgamma / dbeta and dx on the native kernels.
  cannet::group_norm_nhwc(x, weight, bias, groups, eps, relu) -> (y, stats)
      F.group_norm(x, groups, weight, bias, eps) [+ ReLU] of an NHWC bf16/fp16 map, C % 8 == 0, C % groups == 0, fp32
      parameters (csrc/groupnorm.hip); groups == C is instance norm.  Statistics per (sample, group) from double sums
      in a fixed order: stats = fp32 [N, groups, 3] (mean, biased variance, rstd), not differentiable.  No eval mode
      and no running statistics.  Backward: dz = dY masked by the stored y > 0, then dgamma / dbeta and dx on the
      native kernels.
  cannet::adaptive_avg_pool_nhwc(x, oh, ow) -> y
      F.adaptive_avg_pool2d of an NHWC bf16/fp16 map, C % 8 == 0, any sizes >= 1 (bins overlap when H % oh != 0,
      oh > H is legal): fp32 sum of the bin / float(count), one rounding (csrc/resample.hip).  Backward: a gather
      over the bins that hold each input pixel.
  cannet::resize_bilinear_nhwc(x, oh, ow, align_corners) -> y
      F.interpolate(x, (oh, ow), mode="bilinear", align_corners=...) of an NHWC bf16/fp16 map, C % 8 == 0, up or
      down, any ratio; taps from float64 host tables, fma blends in fp32, one rounding.  Backward: the exact adjoint
      as a gather (no atomics, fixed order).
  cannet::sgd_momentum_(param, momentum_buf, grad, lr, momentum, grad_scale) -> ()
      in-place fused SGD with momentum on contiguous fp32 tensors (torch.optim.SGD semantics, weight decay 0,
      dampening 0: buf = momentum * buf + grad_scale * grad; param -= lr * buf), one kernel.
  cannet::adam_(param, exp_avg, exp_avg_sq, grad, step, lr, beta1, beta2, eps, weight_decay, decoupled,
                grad_scale) -> ()
      in-place fused Adam (decoupled=False: torch.optim.Adam, weight decay added to the gradient) or AdamW
      (decoupled=True) on contiguous fp32 tensors, one kernel; ``step`` is the 1-based step of this call (the bias
      corrections are 1 - beta^step); no amsgrad, no maximize.

``Conv2dNHWC`` / ``Conv2dThinNHWC`` / ``Conv2dDown2NHWC`` / ``ConvTranspose2dUp2NHWC`` / ``BatchNorm2dNHWC`` /
``GroupNorm2dNHWC`` / ``InstanceNorm2dNHWC`` / ``ReluMaxPool2x2`` are nn.Module wrappers with fp32 master parameters; ``AdaptiveAvgPool2dNHWC`` / ``ResizeBilinearNHWC`` wrap the two resampling ops.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _ext
from . import batchnorm as BN
from . import conv as C
from . import groupnorm as GN
from . import resample as RS

_LIB = "cannet"


def _conv_check(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                dilation: int) -> Tuple[int, int, int]:
    if x.dim() != 4:
        raise ValueError("x must be NHWC [N,H,W,Ci]")
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[2] not in (1, 3, 5, 7):
        raise ValueError("weight must be [Co,Ci,k,k] with k = 1, 3, 5 or 7")
    co, ci, k, _ = weight.shape
    if k > 3 and not 1 <= dilation * (k // 2) <= C.LARGE_MAX_REACH:
        raise ValueError(f"a {k}x{k} layer needs dilation * {k // 2} <= {C.LARGE_MAX_REACH}, got dilation {dilation}")
    if x.shape[-1] != ci:
        raise ValueError(f"x has {x.shape[-1]} channels, weight expects {ci}")
    if ci % 16 or co % 16 or ci == 0 or co == 0:
        raise ValueError("cannet::conv2d_nhwc needs Ci and Co multiples of 16")
    if x.dtype not in C.ACT_DTYPES:
        raise ValueError(f"x must be bf16 or fp16, got {x.dtype}")
    if weight.dtype != torch.float32:
        raise ValueError("weight must be the fp32 master tensor")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != co):
        raise ValueError("bias must be fp32 [Co]")
    return ci, co, k


@torch.library.custom_op(f"{_LIB}::conv2d_nhwc", mutates_args=())
def conv2d_nhwc(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], dilation: int = 1,
                relu: bool = True) -> torch.Tensor:
    ci, co, k = _conv_check(x, weight, bias, dilation)
    x = x.contiguous()
    wp = C.pack_weight_fwd(weight, x.dtype)
    if bias is None:
        if relu:
            bias = torch.zeros(co, dtype=torch.float32, device=x.device)
            epi = C.EPI_BIAS_RELU
        else:
            epi = C.EPI_NONE
    else:
        bias = bias.detach().contiguous()
        epi = C.EPI_BIAS_RELU if relu else C.EPI_BIAS
    if k > 3 or C.small_channels(ci, co):
        return C.conv_small(x, wp, bias, ksize=k, dil=dilation, epi=epi)
    return C.conv_igemm(x, wp, bias, ksize=k, dil=dilation, epi=epi)


@conv2d_nhwc.register_fake
def _(x, weight, bias, dilation=1, relu=True):
    _conv_check(x, weight, bias, dilation)
    return x.new_empty(*x.shape[:3], weight.shape[0])


@torch.library.custom_op(f"{_LIB}::conv2d_nhwc_backward", mutates_args=())
def conv2d_nhwc_backward(dy: torch.Tensor, x: torch.Tensor, y: torch.Tensor, weight: torch.Tensor, dilation: int,
                         relu: bool, need_bias: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dweight, dbias) of conv2d_nhwc; dbias is an empty tensor when need_bias is False."""
    co, ci, k, _ = weight.shape
    dz = dy.to(x.dtype)
    if relu:
        dz = torch.where(y > 0, dz, torch.zeros((), dtype=dz.dtype, device=dz.device))
    dz = dz.contiguous()
    small = k > 3 or C.small_channels(ci, co)
    conv, wgrad = (C.conv_small, C.conv_small_wgrad) if small else (C.conv_igemm, C.conv_wgrad)
    dx = conv(dz, C.pack_weight_dgrad(weight, x.dtype), None, ksize=k, dil=dilation, epi=C.EPI_NONE)
    dw = torch.empty(co, ci, k, k, dtype=torch.float32, device=x.device)
    db = torch.empty(co if need_bias else 0, dtype=torch.float32, device=x.device)
    wgrad(dz, x.contiguous(), dw, db if need_bias else None, ksize=k, dil=dilation)
    return dx, dw, db


@conv2d_nhwc_backward.register_fake
def _(dy, x, y, weight, dilation, relu, need_bias):
    co = weight.shape[0]
    return (x.new_empty(x.shape), weight.new_empty(weight.shape), weight.new_empty(co if need_bias else 0))


def _conv_setup(ctx, inputs, output):
    x, weight, bias, dilation, relu = inputs
    ctx.save_for_backward(x, weight, output)
    ctx.dilation, ctx.relu, ctx.has_bias = dilation, relu, bias is not None


def _conv_bwd(ctx, dy):
    x, weight, y = ctx.saved_tensors
    dx, dw, db = conv2d_nhwc_backward(dy, x, y, weight, ctx.dilation, ctx.relu, ctx.has_bias)
    return dx, dw, (db if ctx.has_bias else None), None, None


conv2d_nhwc.register_autograd(_conv_bwd, setup_context=_conv_setup)


def _thin_check(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], dilation: int,
                fp32_out: bool) -> Tuple[int, int, int]:
    if x.dim() != 4:
        raise ValueError("x must be NHWC [N,H,W,Ci]")
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[2] not in (1, 3):
        raise ValueError("weight must be [Co,Ci,k,k] with k = 1 or 3")
    co, ci, k, _ = weight.shape
    if x.shape[-1] != ci:
        raise ValueError(f"x has {x.shape[-1]} channels, weight expects {ci}")
    if not C.thin_channels(ci, co):
        raise ValueError(f"cannet::conv2d_thin_nhwc needs exactly one of Ci, Co in 1 .. {C.THIN_MAX} and the other a "
                         f"multiple of 16, got {ci} -> {co}")
    if not 1 <= dilation <= C.SMALL_MAX_DIL:
        raise ValueError(f"dilation must be 1 .. {C.SMALL_MAX_DIL}, got {dilation}")
    if fp32_out and co > C.THIN_MAX:
        raise ValueError("fp32_out needs a thin Co")
    if x.dtype not in C.ACT_DTYPES:
        raise ValueError(f"x must be bf16 or fp16, got {x.dtype}")
    if weight.dtype != torch.float32:
        raise ValueError("weight must be the fp32 master tensor")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != co):
        raise ValueError("bias must be fp32 [Co]")
    return ci, co, k


@torch.library.custom_op(f"{_LIB}::conv2d_thin_nhwc", mutates_args=())
def conv2d_thin_nhwc(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], dilation: int = 1,
                     relu: bool = True, fp32_out: bool = False) -> torch.Tensor:
    ci, co, k = _thin_check(x, weight, bias, dilation, fp32_out)
    x = x.contiguous()
    wp = C.pack_weight_fwd(weight, x.dtype)
    if bias is None:
        if relu:
            bias = torch.zeros(co, dtype=torch.float32, device=x.device)
            epi = C.EPI_BIAS_RELU
        else:
            epi = C.EPI_NONE
    else:
        bias = bias.detach().contiguous()
        epi = C.EPI_BIAS_RELU if relu else C.EPI_BIAS
    return C.conv_thin(x, wp, bias, ksize=k, dil=dilation, epi=epi, fp32_out=fp32_out)


@conv2d_thin_nhwc.register_fake
def _(x, weight, bias, dilation=1, relu=True, fp32_out=False):
    _thin_check(x, weight, bias, dilation, fp32_out)
    return x.new_empty(*x.shape[:3], weight.shape[0], dtype=torch.float32 if fp32_out else x.dtype)


@torch.library.custom_op(f"{_LIB}::conv2d_thin_nhwc_backward", mutates_args=())
def conv2d_thin_nhwc_backward(dy: torch.Tensor, x: torch.Tensor, y: torch.Tensor, weight: torch.Tensor, dilation: int,
                              relu: bool, need_bias: bool,
                              need_dx: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dweight, dbias) of conv2d_thin_nhwc; dx / dbias are empty tensors when need_dx / need_bias is False."""
    co, ci, k, _ = weight.shape
    dz = dy.to(x.dtype)
    if relu:
        dz = torch.where(y > 0, dz, torch.zeros((), dtype=dz.dtype, device=dz.device))
    dz = dz.contiguous()
    if need_dx:
        dx = C.conv_thin(dz, C.pack_weight_dgrad(weight, x.dtype), None, ksize=k, dil=dilation, epi=C.EPI_NONE)
    else:
        dx = x.new_empty(0)
    dw = torch.empty(co, ci, k, k, dtype=torch.float32, device=x.device)
    db = torch.empty(co if need_bias else 0, dtype=torch.float32, device=x.device)
    C.conv_thin_wgrad(dz, x.contiguous(), dw, db if need_bias else None, ksize=k, dil=dilation)
    return dx, dw, db


@conv2d_thin_nhwc_backward.register_fake
def _(dy, x, y, weight, dilation, relu, need_bias, need_dx):
    co = weight.shape[0]
    return (x.new_empty(x.shape if need_dx else (0,)), weight.new_empty(weight.shape),
            weight.new_empty(co if need_bias else 0))


def _thin_setup(ctx, inputs, output):
    x, weight, bias, dilation, relu, _ = inputs
    ctx.save_for_backward(x, weight, output)
    ctx.dilation, ctx.relu, ctx.has_bias = dilation, relu, bias is not None


def _thin_bwd(ctx, dy):
    x, weight, y = ctx.saved_tensors
    need_dx = ctx.needs_input_grad[0]                    # an image normally needs no gradient
    dx, dw, db = conv2d_thin_nhwc_backward(dy, x, y, weight, ctx.dilation, ctx.relu, ctx.has_bias, need_dx)
    return (dx if need_dx else None), dw, (db if ctx.has_bias else None), None, None, None


conv2d_thin_nhwc.register_autograd(_thin_bwd, setup_context=_thin_setup)


def _s2_check(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], up: bool) -> Tuple[int, int, int]:
    """(ci, co, k) of a stride-2 layer; weight [Co,Ci,k,k] (down) or [Ci,Co,k,k] (up, nn.ConvTranspose2d's layout)."""
    name = "cannet::conv_transpose2d_up2_nhwc" if up else "cannet::conv2d_down2_nhwc"
    if x.dim() != 4:
        raise ValueError("x must be NHWC [N,H,W,Ci]")
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or not 1 <= weight.shape[2] <= C.S2_MAX_K:
        raise ValueError(f"weight must be 4-d with k x k taps, k = 1 .. {C.S2_MAX_K}")
    k = weight.shape[2]
    ci, co = (weight.shape[0], weight.shape[1]) if up else (weight.shape[1], weight.shape[0])
    if x.shape[-1] != ci:
        raise ValueError(f"x has {x.shape[-1]} channels, weight expects {ci}")
    if ci % 16 or co % 16 or ci == 0 or co == 0:
        raise ValueError(f"{name} needs Ci and Co multiples of 16")
    if min(x.shape[:3]) < 1 or (not up and (x.shape[1] % 2 or x.shape[2] % 2)):
        raise ValueError(f"{name} needs a non-empty map" + ("" if up else " of even H and W"))
    if x.dtype not in C.ACT_DTYPES:
        raise ValueError(f"x must be bf16 or fp16, got {x.dtype}")
    if weight.dtype != torch.float32:
        raise ValueError("weight must be the fp32 master tensor")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != co):
        raise ValueError("bias must be fp32 [Co]")
    return ci, co, k


def _s2_epilogue(bias: Optional[torch.Tensor], relu: bool, co: int, device):
    if bias is None:
        if relu:
            return torch.zeros(co, dtype=torch.float32, device=device), C.EPI_BIAS_RELU
        return None, C.EPI_NONE
    return bias.detach().contiguous(), (C.EPI_BIAS_RELU if relu else C.EPI_BIAS)


def _s2_dz(dy: torch.Tensor, y: torch.Tensor, relu: bool) -> torch.Tensor:
    dz = dy.to(y.dtype)
    if relu:
        dz = torch.where(y > 0, dz, torch.zeros((), dtype=dz.dtype, device=dz.device))
    return dz.contiguous()


@torch.library.custom_op(f"{_LIB}::conv2d_down2_nhwc", mutates_args=())
def conv2d_down2_nhwc(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                      relu: bool = True) -> torch.Tensor:
    ci, co, k = _s2_check(x, weight, bias, False)
    x = x.contiguous()
    bias, epi = _s2_epilogue(bias, relu, co, x.device)
    return C.conv_down2(x, C.pack_weight_fwd(weight, x.dtype), bias, ksize=k, epi=epi)


@conv2d_down2_nhwc.register_fake
def _(x, weight, bias, relu=True):
    _s2_check(x, weight, bias, False)
    return x.new_empty(x.shape[0], x.shape[1] // 2, x.shape[2] // 2, weight.shape[0])


@torch.library.custom_op(f"{_LIB}::conv2d_down2_nhwc_backward", mutates_args=())
def conv2d_down2_nhwc_backward(dy: torch.Tensor, x: torch.Tensor, y: torch.Tensor, weight: torch.Tensor, relu: bool,
                               need_bias: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dweight, dbias) of conv2d_down2_nhwc; dbias is an empty tensor when need_bias is False."""
    co, ci, k, _ = weight.shape
    dz = _s2_dz(dy, y, relu)
    # the data gradient is the transposed conv Co -> Ci whose weight, in nn.ConvTranspose2d's layout, is `weight`
    dx = C.conv_up2(dz, C.pack_weight_up(weight, x.dtype), None, ksize=k, epi=C.EPI_NONE)
    dw = torch.empty(co, ci, k, k, dtype=torch.float32, device=x.device)
    db = torch.empty(co if need_bias else 0, dtype=torch.float32, device=x.device)
    C.conv_s2_wgrad(dz, x.contiguous(), dw, db if need_bias else None, ksize=k, bias_of="small")
    return dx, dw, db


@conv2d_down2_nhwc_backward.register_fake
def _(dy, x, y, weight, relu, need_bias):
    return (x.new_empty(x.shape), weight.new_empty(weight.shape),
            weight.new_empty(weight.shape[0] if need_bias else 0))


@torch.library.custom_op(f"{_LIB}::conv_transpose2d_up2_nhwc", mutates_args=())
def conv_transpose2d_up2_nhwc(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                              relu: bool = True) -> torch.Tensor:
    ci, co, k = _s2_check(x, weight, bias, True)
    x = x.contiguous()
    bias, epi = _s2_epilogue(bias, relu, co, x.device)
    return C.conv_up2(x, C.pack_weight_up(weight, x.dtype), bias, ksize=k, epi=epi)


@conv_transpose2d_up2_nhwc.register_fake
def _(x, weight, bias, relu=True):
    _s2_check(x, weight, bias, True)
    return x.new_empty(x.shape[0], 2 * x.shape[1], 2 * x.shape[2], weight.shape[1])


@torch.library.custom_op(f"{_LIB}::conv_transpose2d_up2_nhwc_backward", mutates_args=())
def conv_transpose2d_up2_nhwc_backward(dy: torch.Tensor, x: torch.Tensor, y: torch.Tensor, weight: torch.Tensor,
                                       relu: bool, need_bias: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dweight, dbias) of conv_transpose2d_up2_nhwc; dbias is an empty tensor when need_bias is False."""
    ci, co, k, _ = weight.shape
    dz = _s2_dz(dy, y, relu)
    # the data gradient is the down-sampling conv Co -> Ci with weight[ci][co] as its [out][in] weight
    dx = C.conv_down2(dz, C.pack_weight_fwd(weight, x.dtype), None, ksize=k, epi=C.EPI_NONE)
    dw = torch.empty(ci, co, k, k, dtype=torch.float32, device=x.device)
    db = torch.empty(co if need_bias else 0, dtype=torch.float32, device=x.device)
    C.conv_s2_wgrad(x.contiguous(), dz, dw, db if need_bias else None, ksize=k, bias_of="big")
    return dx, dw, db


@conv_transpose2d_up2_nhwc_backward.register_fake
def _(dy, x, y, weight, relu, need_bias):
    return (x.new_empty(x.shape), weight.new_empty(weight.shape),
            weight.new_empty(weight.shape[1] if need_bias else 0))


def _s2_setup(ctx, inputs, output):
    x, weight, bias, relu = inputs
    ctx.save_for_backward(x, weight, output)
    ctx.relu, ctx.has_bias = relu, bias is not None


def _down2_bwd(ctx, dy):
    x, weight, y = ctx.saved_tensors
    dx, dw, db = conv2d_down2_nhwc_backward(dy, x, y, weight, ctx.relu, ctx.has_bias)
    return dx, dw, (db if ctx.has_bias else None), None


def _up2_bwd(ctx, dy):
    x, weight, y = ctx.saved_tensors
    dx, dw, db = conv_transpose2d_up2_nhwc_backward(dy, x, y, weight, ctx.relu, ctx.has_bias)
    return dx, dw, (db if ctx.has_bias else None), None


conv2d_down2_nhwc.register_autograd(_down2_bwd, setup_context=_s2_setup)
conv_transpose2d_up2_nhwc.register_autograd(_up2_bwd, setup_context=_s2_setup)


@torch.library.custom_op(f"{_LIB}::relu_max_pool2x2", mutates_args=())
def relu_max_pool2x2(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    y, codes = C.maxpool_codes(x.contiguous())
    return y.clamp_min_(0), codes          # relu(max): a window whose max is <= 0 pools to 0 (its code is 0)


@relu_max_pool2x2.register_fake
def _(x):
    n, h, w, c = x.shape
    if h % 2 or w % 2 or c % 8:
        raise ValueError("max-pool needs even H, W and C % 8 == 0")
    return x.new_empty(n, h // 2, w // 2, c), x.new_empty(n, h // 2, w // 2, c // 8, dtype=torch.int32)


@torch.library.custom_op(f"{_LIB}::relu_max_pool2x2_backward", mutates_args=())
def relu_max_pool2x2_backward(dy: torch.Tensor, codes: torch.Tensor) -> torch.Tensor:
    return C.maxpool_bwd_codes(codes, dy.contiguous())


@relu_max_pool2x2_backward.register_fake
def _(dy, codes):
    n, h, w, c = dy.shape
    return dy.new_empty(n, 2 * h, 2 * w, c)


def _pool_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.mark_non_differentiable(output[1])


def _pool_bwd(ctx, dy, dcodes):
    (codes,) = ctx.saved_tensors
    return relu_max_pool2x2_backward(dy, codes)


relu_max_pool2x2.register_autograd(_pool_bwd, setup_context=_pool_setup)


def _bn_check(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, running_mean: Optional[torch.Tensor],
              running_var: Optional[torch.Tensor], training: bool) -> int:
    if x.dim() != 4:
        raise ValueError("x must be NHWC [N,H,W,C]")
    c = x.shape[-1]
    if c == 0 or c % 8:
        raise ValueError("cannet::batch_norm_nhwc needs C a multiple of 8")
    if x.dtype not in C.ACT_DTYPES:
        raise ValueError(f"x must be bf16 or fp16, got {x.dtype}")
    vecs = [(weight, "weight"), (bias, "bias")]
    if not training:
        vecs += [(running_mean, "running_mean"), (running_var, "running_var")]
    for t, name in vecs:
        if t is None or t.dtype != torch.float32 or t.numel() != c:
            raise ValueError(f"{name} must be fp32 [{c}]")
    return c


@torch.library.custom_op(f"{_LIB}::batch_norm_nhwc", mutates_args=())
def batch_norm_nhwc(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, running_mean: Optional[torch.Tensor],
                    running_var: Optional[torch.Tensor], training: bool, eps: float = 1e-5,
                    relu: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    _bn_check(x, weight, bias, running_mean, running_var, training)
    return BN.bn_forward(x.contiguous(), weight, bias, running_mean, running_var, training, eps, relu)


@batch_norm_nhwc.register_fake
def _(x, weight, bias, running_mean, running_var, training, eps=1e-5, relu=True):
    c = _bn_check(x, weight, bias, running_mean, running_var, training)
    return x.new_empty(x.shape), x.new_empty(3, c, dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::batch_norm_nhwc_backward", mutates_args=())
def batch_norm_nhwc_backward(dy: torch.Tensor, x: torch.Tensor, y: torch.Tensor, weight: torch.Tensor,
                             stats: torch.Tensor, training: bool,
                             relu: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dweight, dbias) of batch_norm_nhwc."""
    dx, dg, db = BN.bn_backward(dy.to(x.dtype).contiguous(), x.contiguous(), y, weight, stats, training, relu)
    return dx, dg.clone(), db.clone()           # dg / db are rows of one workspace tensor: outputs own their memory


@batch_norm_nhwc_backward.register_fake
def _(dy, x, y, weight, stats, training, relu):
    return x.new_empty(x.shape), weight.new_empty(weight.shape), weight.new_empty(weight.shape)


def _bn_setup(ctx, inputs, output):
    x, weight, _, _, _, training, _, relu = inputs
    y, stats = output
    ctx.save_for_backward(x, y, weight, stats)
    ctx.mark_non_differentiable(stats)
    ctx.training, ctx.relu = training, relu


def _bn_bwd(ctx, dy, dstats):
    x, y, weight, stats = ctx.saved_tensors
    dx, dg, db = batch_norm_nhwc_backward(dy, x, y, weight, stats, ctx.training, ctx.relu)
    return dx, dg, db, None, None, None, None, None


batch_norm_nhwc.register_autograd(_bn_bwd, setup_context=_bn_setup)


def _gn_check(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, groups: int) -> Tuple[int, int]:
    if x.dim() != 4:
        raise ValueError("x must be NHWC [N,H,W,C]")
    n, h, w, c = x.shape
    if c == 0 or c % 8:
        raise ValueError("cannet::group_norm_nhwc needs C a multiple of 8")
    if groups < 1 or c % groups:
        raise ValueError(f"groups={groups} must divide C={c}")
    if h * w * (c // groups) < 2:
        raise ValueError("group norm needs more than one value per (sample, group)")
    if x.dtype not in C.ACT_DTYPES:
        raise ValueError(f"x must be bf16 or fp16, got {x.dtype}")
    for t, name in ((weight, "weight"), (bias, "bias")):
        if t.dtype != torch.float32 or t.numel() != c:
            raise ValueError(f"{name} must be fp32 [{c}]")
    return n, c


@torch.library.custom_op(f"{_LIB}::group_norm_nhwc", mutates_args=())
def group_norm_nhwc(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, groups: int, eps: float = 1e-5,
                    relu: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    _gn_check(x, weight, bias, groups)
    return GN.gn_forward(x.contiguous(), weight, bias, groups, eps, relu)


@group_norm_nhwc.register_fake
def _(x, weight, bias, groups, eps=1e-5, relu=True):
    n, _ = _gn_check(x, weight, bias, groups)
    return x.new_empty(x.shape), x.new_empty(n, groups, 3, dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::group_norm_nhwc_backward", mutates_args=())
def group_norm_nhwc_backward(dy: torch.Tensor, x: torch.Tensor, y: torch.Tensor, weight: torch.Tensor,
                             stats: torch.Tensor, groups: int,
                             relu: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dweight, dbias) of group_norm_nhwc."""
    dx, dg, db = GN.gn_backward(dy.to(x.dtype).contiguous(), x.contiguous(), y, weight, stats, groups, relu)
    return dx, dg.clone(), db.clone()           # dg / db are rows of one workspace tensor: outputs own their memory


@group_norm_nhwc_backward.register_fake
def _(dy, x, y, weight, stats, groups, relu):
    return x.new_empty(x.shape), weight.new_empty(weight.shape), weight.new_empty(weight.shape)


def _gn_setup(ctx, inputs, output):
    x, weight, _, groups, _, relu = inputs
    y, stats = output
    ctx.save_for_backward(x, y, weight, stats)
    ctx.mark_non_differentiable(stats)
    ctx.groups, ctx.relu = groups, relu


def _gn_bwd(ctx, dy, dstats):
    x, y, weight, stats = ctx.saved_tensors
    dx, dg, db = group_norm_nhwc_backward(dy, x, y, weight, stats, ctx.groups, ctx.relu)
    return dx, dg, db, None, None, None


group_norm_nhwc.register_autograd(_gn_bwd, setup_context=_gn_setup)


def _resample_check(x: torch.Tensor, oh: int, ow: int) -> None:
    if x.dim() != 4:
        raise ValueError("x must be NHWC [N,H,W,C]")
    if x.shape[-1] == 0 or x.shape[-1] % 8:
        raise ValueError("the resampling ops need C a multiple of 8")
    if x.dtype not in C.ACT_DTYPES:
        raise ValueError(f"x must be bf16 or fp16, got {x.dtype}")
    if min(*x.shape, oh, ow) < 1:
        raise ValueError("every size must be >= 1")


@torch.library.custom_op(f"{_LIB}::adaptive_avg_pool_nhwc", mutates_args=())
def adaptive_avg_pool_nhwc(x: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    _resample_check(x, oh, ow)
    return RS.adaptive_avg_pool(x.contiguous(), oh, ow)


@adaptive_avg_pool_nhwc.register_fake
def _(x, oh, ow):
    _resample_check(x, oh, ow)
    return x.new_empty(x.shape[0], oh, ow, x.shape[3])


@torch.library.custom_op(f"{_LIB}::adaptive_avg_pool_nhwc_backward", mutates_args=())
def adaptive_avg_pool_nhwc_backward(dy: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """dx [N,h,w,C] of adaptive_avg_pool_nhwc."""
    return RS.adaptive_avg_pool_backward(dy.contiguous(), h, w)


@adaptive_avg_pool_nhwc_backward.register_fake
def _(dy, h, w):
    return dy.new_empty(dy.shape[0], h, w, dy.shape[3])


def _apool_setup(ctx, inputs, output):
    ctx.hw = tuple(inputs[0].shape[1:3])


def _apool_bwd(ctx, dy):
    return adaptive_avg_pool_nhwc_backward(dy, *ctx.hw), None, None


adaptive_avg_pool_nhwc.register_autograd(_apool_bwd, setup_context=_apool_setup)


@torch.library.custom_op(f"{_LIB}::resize_bilinear_nhwc", mutates_args=())
def resize_bilinear_nhwc(x: torch.Tensor, oh: int, ow: int, align_corners: bool = False) -> torch.Tensor:
    _resample_check(x, oh, ow)
    return RS.resize_bilinear(x.contiguous(), oh, ow, align_corners)


@resize_bilinear_nhwc.register_fake
def _(x, oh, ow, align_corners=False):
    _resample_check(x, oh, ow)
    return x.new_empty(x.shape[0], oh, ow, x.shape[3])


@torch.library.custom_op(f"{_LIB}::resize_bilinear_nhwc_backward", mutates_args=())
def resize_bilinear_nhwc_backward(dy: torch.Tensor, h: int, w: int, align_corners: bool) -> torch.Tensor:
    """dx [N,h,w,C] of resize_bilinear_nhwc."""
    return RS.resize_bilinear_backward(dy.contiguous(), h, w, align_corners)


@resize_bilinear_nhwc_backward.register_fake
def _(dy, h, w, align_corners):
    return dy.new_empty(dy.shape[0], h, w, dy.shape[3])


def _resize_setup(ctx, inputs, output):
    ctx.hw, ctx.align_corners = tuple(inputs[0].shape[1:3]), inputs[3]


def _resize_bwd(ctx, dy):
    return resize_bilinear_nhwc_backward(dy, *ctx.hw, ctx.align_corners), None, None, None


resize_bilinear_nhwc.register_autograd(_resize_bwd, setup_context=_resize_setup)


@torch.library.custom_op(f"{_LIB}::sgd_momentum_", mutates_args=("param", "momentum_buf"))
def sgd_momentum_(param: torch.Tensor, momentum_buf: torch.Tensor, grad: torch.Tensor, lr: float, momentum: float,
                  grad_scale: float = 1.0) -> None:
    for t, name in ((param, "param"), (momentum_buf, "momentum_buf"), (grad, "grad")):
        if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"{name} must be a contiguous fp32 GPU tensor")
    if not (param.numel() == momentum_buf.numel() == grad.numel()):
        raise ValueError("param / momentum_buf / grad sizes differ")
    n = param.numel()
    if n == 0:
        return
    if any(t.data_ptr() % 16 for t in (param, momentum_buf, grad)):
        momentum_buf.mul_(momentum).add_(grad, alpha=grad_scale)      # float4 kernel needs 16-B alignment
        param.add_(momentum_buf, alpha=-lr)
        return
    Cx = _ext.require()
    # the arena kernel works on float4 groups; a ragged tail (n % 4) goes through ATen
    n4 = n - n % 4
    if n4:
        Cx.sgd_momentum(param.data_ptr(), momentum_buf.data_ptr(), grad.data_ptr(), n4, float(lr), float(momentum),
                        float(grad_scale), 0, 0, 0, _ext.stream_ptr(param.device))
    if n4 < n:
        b, g, p = momentum_buf.view(-1)[n4:], grad.view(-1)[n4:], param.view(-1)[n4:]
        b.mul_(momentum).add_(g, alpha=grad_scale)
        p.add_(b, alpha=-lr)


@sgd_momentum_.register_fake
def _(param, momentum_buf, grad, lr, momentum, grad_scale=1.0):
    return None


def _adam_aten(param, exp_avg, exp_avg_sq, grad, step, lr, beta1, beta2, eps, weight_decay, decoupled, grad_scale):
    """torch.optim.Adam / AdamW's single-tensor update in ATen ops (the fallback for tensors off 16-byte alignment)."""
    g = grad * grad_scale
    if decoupled:
        param.mul_(1.0 - lr * weight_decay)
    elif weight_decay != 0:
        g = g.add(param, alpha=weight_decay)
    exp_avg.lerp_(g, 1.0 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    denom = (exp_avg_sq.sqrt() / (1.0 - beta2 ** step) ** 0.5).add_(eps)
    param.addcdiv_(exp_avg, denom, value=-lr / (1.0 - beta1 ** step))


@torch.library.custom_op(f"{_LIB}::adam_", mutates_args=("param", "exp_avg", "exp_avg_sq"))
def adam_(param: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, grad: torch.Tensor, step: int,
          lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
          decoupled: bool = False, grad_scale: float = 1.0) -> None:
    ts = ((param, "param"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (grad, "grad"))
    for t, name in ts:
        if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"{name} must be a contiguous fp32 GPU tensor")
    if not (param.numel() == exp_avg.numel() == exp_avg_sq.numel() == grad.numel()):
        raise ValueError("param / exp_avg / exp_avg_sq / grad sizes differ")
    if step < 1:
        raise ValueError("step is the 1-based step of this call")
    n = param.numel()
    if n == 0:
        return
    hp = (step, float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), bool(decoupled),
          float(grad_scale))
    if any(t.data_ptr() % 16 for t, _ in ts):
        _adam_aten(param, exp_avg, exp_avg_sq, grad, *hp)            # as sgd_momentum_: float4 groups need 16 B
        return
    # adam_kernel takes the n % 4 tail itself, so the op is C.adam bit for bit
    _ext.require().adam(param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), grad.data_ptr(), n, hp[1], hp[2],
                        hp[3], hp[4], hp[5], int(hp[6]), hp[7], int(step), 0, 0, 0, _ext.stream_ptr(param.device))


@adam_.register_fake
def _(param, exp_avg, exp_avg_sq, grad, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
      decoupled=False, grad_scale=1.0):
    return None


@torch.library.custom_op(f"{_LIB}::ema_", mutates_args=("ema",))
def ema_(ema: torch.Tensor, param: torch.Tensor, decay: float, warmup: bool = True, step: int = 1) -> None:
    """ema += w (param - ema), w = float32(1 - d), d = min(decay, (1 + n) / (10 + n)) with ``warmup`` (n = step - 1,
    ``step`` the 1-based update of this call), d = decay without: the native step's EMA update (elementwise.hip
    ema_kernel, any size and alignment), bit for bit ``C.ema``."""
    for t, name in ((ema, "ema"), (param, "param")):
        if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"{name} must be a contiguous fp32 GPU tensor")
    if ema.numel() != param.numel():
        raise ValueError("ema / param sizes differ")
    if not 0.0 <= decay < 1.0:
        raise ValueError("decay must be in [0, 1)")
    if step < 1:
        raise ValueError("step is the 1-based update of this call")
    if ema.numel() == 0:
        return
    _ext.require().ema(ema.data_ptr(), param.data_ptr(), ema.numel(), float(decay), int(bool(warmup)), int(step), 0, 0,
                       _ext.stream_ptr(ema.device))


@ema_.register_fake
def _(ema, param, decay, warmup=True, step=1):
    return None


class Conv2dNHWC(nn.Module):
    """nn.Conv2d(ci, co, k, padding=dilation*(k//2), dilation=dilation) [+ ReLU] on NHWC 16-bit activations, run
    by the native MFMA kernels (``torch.ops.cannet.conv2d_nhwc``).  Parameters are fp32 in the PyTorch layout, so
    ``state_dict`` is interchangeable with nn.Conv2d's."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 3, dilation: int = 1,
                 bias: bool = True, relu: bool = True):
        super().__init__()
        if kernel_size not in (1, 3, 5, 7):
            raise ValueError("kernel_size must be 1, 3, 5 or 7")
        self.dilation, self.relu = dilation, relu
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        nn.init.normal_(self.weight, std=0.01)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.ops.cannet.conv2d_nhwc(x, self.weight, self.bias, self.dilation, self.relu)


class Conv2dThinNHWC(nn.Module):
    """Conv2dNHWC for a stem or a head (``torch.ops.cannet.conv2d_thin_nhwc``): exactly one of in_channels /
    out_channels is 1 .. 8, the other a multiple of 16.  Parameters are fp32 in the PyTorch layout, so ``state_dict``
    is interchangeable with nn.Conv2d's.  fp32_out (thin out_channels): the output is fp32."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 3, dilation: int = 1,
                 bias: bool = True, relu: bool = True, fp32_out: bool = False):
        super().__init__()
        if kernel_size not in (1, 3):
            raise ValueError("kernel_size must be 1 or 3")
        if not C.thin_channels(in_channels, out_channels):
            raise ValueError("exactly one of in_channels / out_channels must be 1 .. 8, the other a multiple of 16")
        if fp32_out and out_channels > C.THIN_MAX:
            raise ValueError("fp32_out needs thin out_channels")
        self.dilation, self.relu, self.fp32_out = dilation, relu, fp32_out
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        nn.init.normal_(self.weight, std=0.01)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.ops.cannet.conv2d_thin_nhwc(x, self.weight, self.bias, self.dilation, self.relu, self.fp32_out)


class Conv2dDown2NHWC(nn.Module):
    """nn.Conv2d(ci, co, k, stride=2, padding=(k - 1) // 2) [+ ReLU] on NHWC 16-bit activations of even H and W
    (``torch.ops.cannet.conv2d_down2_nhwc``), k = 1 .. 4.  Parameters are fp32 in the PyTorch layout, so ``state_dict``
    is interchangeable with that nn.Conv2d's."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 3, bias: bool = True, relu: bool = True):
        super().__init__()
        if not 1 <= kernel_size <= C.S2_MAX_K:
            raise ValueError(f"kernel_size must be 1 .. {C.S2_MAX_K}")
        self.relu = relu
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        nn.init.normal_(self.weight, std=0.01)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.ops.cannet.conv2d_down2_nhwc(x, self.weight, self.bias, self.relu)


class ConvTranspose2dUp2NHWC(nn.Module):
    """nn.ConvTranspose2d(ci, co, k, stride=2, padding=(k - 1) // 2, output_padding=k % 2) [+ ReLU] on NHWC 16-bit
    activations (``torch.ops.cannet.conv_transpose2d_up2_nhwc``), k = 1 .. 4: the output is exactly twice the input.
    Parameters are fp32 in nn.ConvTranspose2d's layout ([in, out, k, k]), so ``state_dict`` is interchangeable with
    it."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 2, bias: bool = True, relu: bool = True):
        super().__init__()
        if not 1 <= kernel_size <= C.S2_MAX_K:
            raise ValueError(f"kernel_size must be 1 .. {C.S2_MAX_K}")
        self.relu = relu
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        nn.init.normal_(self.weight, std=0.01)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.ops.cannet.conv_transpose2d_up2_nhwc(x, self.weight, self.bias, self.relu)


class BatchNorm2dNHWC(nn.Module):
    """nn.BatchNorm2d(num_features) [+ ReLU] on NHWC 16-bit activations (``torch.ops.cannet.batch_norm_nhwc``).
    Parameters and buffers carry nn.BatchNorm2d's names and shapes, so ``state_dict`` is interchangeable with it
    (a ``make_layers(batch_norm=True)`` checkpoint loads).  The op is functional; in training this module updates the
    running buffers from the op's stats under ATen's rule (unbiased variance, ``momentum=None``: cumulative average)."""

    def __init__(self, num_features: int, eps: float = 1e-5, momentum: Optional[float] = 0.1, relu: bool = True):
        super().__init__()
        self.num_features, self.eps, self.momentum, self.relu = num_features, eps, momentum, relu
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y, stats = torch.ops.cannet.batch_norm_nhwc(x, self.weight, self.bias, self.running_mean, self.running_var,
                                                    self.training, self.eps, self.relu)
        if self.training:
            with torch.no_grad():
                self.num_batches_tracked += 1
                f = 1.0 / self.num_batches_tracked if self.momentum is None else self.momentum
                m = x.numel() // x.shape[-1]
                self.running_mean.lerp_(stats[0], f)
                self.running_var.lerp_(stats[1] * (m / (m - 1)), f)
        return y


class GroupNorm2dNHWC(nn.Module):
    """nn.GroupNorm(num_groups, num_channels) [+ ReLU] on NHWC 16-bit activations
    (``torch.ops.cannet.group_norm_nhwc``).  Parameters carry nn.GroupNorm's names and shapes, so ``state_dict`` is
    interchangeable with it; with ``affine=False`` the ones / zeros the op reads are non-persistent buffers."""

    def __init__(self, num_groups: int, num_channels: int, eps: float = 1e-5, affine: bool = True, relu: bool = True):
        super().__init__()
        if num_groups < 1 or num_channels % num_groups:
            raise ValueError("num_channels must be divisible by num_groups")
        self.num_groups, self.num_channels, self.eps, self.affine, self.relu = num_groups, num_channels, eps, affine, relu
        if affine:
            self.weight = nn.Parameter(torch.ones(num_channels))
            self.bias = nn.Parameter(torch.zeros(num_channels))
        else:
            self.register_buffer("weight", torch.ones(num_channels), persistent=False)
            self.register_buffer("bias", torch.zeros(num_channels), persistent=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.ops.cannet.group_norm_nhwc(x, self.weight, self.bias, self.num_groups, self.eps, self.relu)[0]


class InstanceNorm2dNHWC(GroupNorm2dNHWC):
    """nn.InstanceNorm2d(num_features, affine=..., track_running_stats=False) [+ ReLU] on NHWC 16-bit activations:
    group norm with one channel per group (SANet's layer after every conv).  ``state_dict`` equals nn.InstanceNorm2d's:
    empty with ``affine=False`` (the default), weight and bias otherwise.  No running statistics."""

    def __init__(self, num_features: int, eps: float = 1e-5, affine: bool = False, relu: bool = True):
        super().__init__(num_features, num_features, eps, affine, relu)


class ReluMaxPool2x2(nn.Module):
    """ReLU followed by a 2x2 / stride-2 max-pool of an NHWC map, as one op (``torch.ops.cannet.relu_max_pool2x2``);
    after a ReLU (Conv2dNHWC(relu=True)) it is the plain max-pool."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.ops.cannet.relu_max_pool2x2(x)[0]


def _pair(v) -> Tuple[int, int]:
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


class AdaptiveAvgPool2dNHWC(nn.Module):
    """nn.AdaptiveAvgPool2d(output_size) on NHWC 16-bit activations (``torch.ops.cannet.adaptive_avg_pool_nhwc``);
    output_size is an int or a pair."""

    def __init__(self, output_size):
        super().__init__()
        self.output_size = _pair(output_size)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.ops.cannet.adaptive_avg_pool_nhwc(x, *self.output_size)


class ResizeBilinearNHWC(nn.Module):
    """nn.Upsample(size, scale_factor, mode="bilinear", align_corners=...) on NHWC 16-bit activations
    (``torch.ops.cannet.resize_bilinear_nhwc``).  Exactly one of size (int or pair) and scale_factor (number or pair)
    is given; with scale_factor the output size is F.interpolate's floor(input size * scale_factor), and the taps are
    those of that size (``recompute_scale_factor=True`` where the two differ, i.e. for fractional factors)."""

    def __init__(self, size=None, scale_factor=None, align_corners: bool = False):
        super().__init__()
        if (size is None) == (scale_factor is None):
            raise ValueError("exactly one of size and scale_factor must be given")
        self.size = None if size is None else _pair(size)
        if scale_factor is None:
            self.scale_factor = None
        else:
            sf = (scale_factor, scale_factor) if isinstance(scale_factor, (int, float)) else tuple(scale_factor)
            self.scale_factor = (float(sf[0]), float(sf[1]))
        self.align_corners = bool(align_corners)

    def output_size(self, h: int, w: int) -> Tuple[int, int]:
        if self.size is not None:
            return self.size
        return int(float(h) * self.scale_factor[0]), int(float(w) * self.scale_factor[1])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        oh, ow = self.output_size(x.shape[1], x.shape[2])
        return torch.ops.cannet.resize_bilinear_nhwc(x, oh, ow, self.align_corners)
