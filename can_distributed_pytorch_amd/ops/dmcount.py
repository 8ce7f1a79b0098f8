"""DM-Count loss (Wang et al., NeurIPS 2020) on head records: csrc/otloss.hip (README, "DM-Count loss").

``dmcount_loss`` is the loss of a density map against a ``PointTarget`` (ops/bayes.py): a count term, an entropic
optimal-transport term (a fixed number of Sinkhorn iterations, two MFMA GEMMs each) and a total-variation term, with
the gradient with respect to the map.  The native step reaches it through ``CANNetExecutor.head_train_dmcount``.
There is no route outside HIP.
"""
from __future__ import annotations

import math

import torch

from . import _ext
from .bayes import PointTarget

LDS_TOO_SMALL = "rc=-41"


def _check_params(reg, iters, ot_weight, tv_weight):
    if not 1 <= reg <= 100:
        raise ValueError(f"reg must be in [1, 100] (the Sinkhorn runs in the plain domain), got {reg!r}")
    if int(iters) != iters or not 1 <= iters <= 1000:
        raise ValueError(f"iters must be an integer in [1, 1000], got {iters!r}")
    for name, v in (("ot_weight", ot_weight), ("tv_weight", tv_weight)):
        if not (v >= 0 and math.isfinite(v)):
            raise ValueError(f"{name} must be finite and >= 0, got {v!r}")


def head_tile(max_count: int) -> int:
    """Heads per block of the iteration kernel: small tiles while there are few heads, so that the grid (head tiles x
    samples) still spreads over the CUs; 64 from 257 heads on."""
    return 16 if max_count <= 64 else 32 if max_count <= 256 else 64


def _launch_loss(C, et, target: PointTarget, reg, iters, ot_weight, tv_weight, g, gpitch, loss_ptr, nf_ptr):
    """The 2 iters + 2 launches on et [n, h, w] (dense).  Returns terms [n, 3]; g [n, h, gpitch] is written in place."""
    n, h, w = target.n, target.h, target.w
    T, M = target.pts.shape[0], h * w
    hp, wp = -(-h // 16) * 16, -(-w // 16) * 16
    tile = head_tile(target.max_count)
    ntiles = -(-target.max_count // tile)
    # one fp32 buffer: Ar [T, wp], Br [T, hp] (rows of 64 bytes and more: 16-byte aligned), then part [n, ntiles, M],
    # u, a, q, beta [n, M], v [T], P [n]
    sizes = (T * wp, T * hp, n * ntiles * M, n * M, n * M, n * M, n * M, T, n)
    buf = torch.empty(sum(sizes), dtype=torch.float32, device=et.device)
    ptrs, off = [], 0
    for sz in sizes:
        ptrs.append(buf.data_ptr() + 4 * off)
        off += sz
    Ar, Br, part, u, a, q, beta, v, Pb = ptrs
    terms = torch.empty(n, 3, dtype=torch.float32, device=et.device)
    try:
        C.dmcount_loss(et.data_ptr(), target.pts.data_ptr(), target.begins.data_ptr(), target.cnt.data_ptr(), n, h, w,
                       T, target.max_count, tile, float(reg), int(iters), float(ot_weight), float(tv_weight),
                       target.ch, target.cw, target.ch // h, Ar, Br, u, v, a, q, beta, Pb, part, g.data_ptr(), gpitch,
                       terms.data_ptr(), loss_ptr, nf_ptr, _ext.stream_ptr(et.device))
    except RuntimeError as e:
        if LDS_TOO_SMALL in str(e):
            raise ValueError(f"a map of {h} x {w} cells is too large for the DM-Count iteration kernel: the whole map "
                             f"and a tile of {tile} heads must fit 64 KiB of LDS") from e
        raise
    return terms


def dmcount_loss(et, target: PointTarget, reg: float = 10.0, iters: int = 100, ot_weight: float = 0.1,
                 tv_weight: float = 0.01, gpitch=None):
    """et [n, h, w] or [n, 1, h, w] fp32 on the GPU -> (loss [1], g like et, terms [n, 3]).  terms holds the unweighted
    (L_c, L_ot, L_tv) of every sample; loss = sum over samples of L_c + ot_weight L_ot + tv_weight L_tv.  gpitch > w:
    g is [n, h, gpitch], the gradient of a width-padded map (zeros from column w on)."""
    C = _ext.require()
    _check_params(reg, iters, ot_weight, tv_weight)
    n, h, w = target.n, target.h, target.w
    if et.dtype != torch.float32 or tuple(et.shape) not in ((n, h, w), (n, 1, h, w)) or not et.is_cuda:
        raise ValueError(f"et must be fp32 [{n}, {h}, {w}] or [{n}, 1, {h}, {w}] on the GPU, got {tuple(et.shape)} "
                         f"{et.dtype}")
    target = target.to(et.device)
    etc = et.contiguous()
    if gpitch is None:
        g = torch.empty_like(etc)
    elif gpitch < w:
        raise ValueError(f"gpitch {gpitch} < w {w}")
    else:
        g = torch.empty(n, h, gpitch, dtype=torch.float32, device=et.device)
    loss = torch.empty(1, dtype=torch.float32, device=et.device)
    terms = _launch_loss(C, etc, target, reg, iters, ot_weight, tv_weight, g, g.shape[-1], loss.data_ptr(), 0)
    return loss, g, terms
