"""Native CANNet executor: a static, hand-scheduled forward/backward over the
gfx950 kernels (no tracing compiler, no autograd graph of ATen ops).

Reference math: model/CANNet.py:39-91 (forward), the backward is what
autograd derives for it in the reference (SURVEY §2.5 kernel inventory).

Data layout: NHWC 16-bit activations (bf16 by default, fp16 optional: one
element type for every activation / weight pack of the executor), fp32
master weights in the model's own nn.Parameters, 16-bit packed weight copies
(forward + flipped dgrad layouts) refreshed by one pack launch whenever the
fp32 weights change.

Forward (training) saves exactly what the backward needs: every conv input
(NHWC bf16), the max-pool codes of the three pools (4-bit first-max one-hots:
the full-resolution pre-pool activations are never stored), the context
cell tables and the sigmoid maps w_S (linearised context module: c_S is
never formed).
Backward (per layer, reverse order) = weight-gradient (split-pixel MFMA +
deterministic slab reduction) + data-gradient (same MFMA kernel as forward,
flipped weights, ReLU mask / maxpool-backward fused), and after each layer's
gradients are written a ``on_grad_ready(param_indices)`` callback fires so
a bucketed reducer can start all-reducing while the remaining layers run.

Ragged widths: an input whose width is not a multiple of 64 leaves some resolution level with a width that is not
a multiple of 8 (1016 -> 508 -> 254 -> 127), where the row-ring / tap-ring kernels and the fused pool epilogues do
not apply (round 4: 680x1016 ran 15 % below 768x1024 in TF/s).  With dispatch pad_width (default) the executor runs
such a batch as a WIDTH-PADDED map: the row pitch is the width rounded up to 64 (every level a multiple of 8), the
extra columns are zero.  Exact, not an approximation: zero columns are what the convs' zero padding reads anyway;
every forward epilogue writes zeros at the padding columns (``wvalid``), so they stay zero level after level; the
data gradients are masked there by the ReLU / max-pool masks of those zero activations, so the weight gradients
see no contribution from them; the context module takes its pooling / upsampling geometry from the valid width;
the head excludes them from the loss and its gradients; the density map is returned at the valid width.

Two ways in:
  * ``executor(x)``            — autograd-compatible (CANNet.forward on GPU):
                                 an autograd.Function whose backward returns
                                 ordinary gradients.
  * ``forward_train / backward_from_head`` — used by the native training step
                                 (engine/native.py): gradients go straight into
                                 caller-provided fp32 buffers (the flat gradient
                                 arena), the head/MSE loss is fused.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from . import _ext
from . import conv as C
from . import dispatch
from .context_exec import ContextSchedule
from ..models.cannet import CONTEXT_SCALES

BF16 = torch.bfloat16
CELL_OFF = {1: 0, 2: 1, 3: 5, 6: 14}


@dataclass
class ConvSpec:
    idx: int                 # position in the executor's conv list
    module: nn.Conv2d
    cin: int
    cout: int
    ksize: int
    dil: int
    first: bool = False
    pool_after: bool = False  # a 2x2 maxpool follows this conv's ReLU
    w_index: int = -1         # index of weight in model.parameters()
    b_index: int = -1


class CANNetExecutor(ContextSchedule):
    def __init__(self, model: nn.Module, dtype: torch.dtype = BF16):
        self.C = _ext.require()
        self.model = model
        self.act = dtype                   # activation / weight-pack element type
        self.dt = C.dt_code(dtype)
        params = list(model.parameters())
        self._plist = params               # parameter list, fixed for the executor's life (the flat arena moves
        #                                    the storage of these same Parameter objects, never replaces them)
        pid = {id(p): i for i, p in enumerate(params)}
        self.n_params = len(params)
        self.front: List[ConvSpec] = []
        mods = list(model.frontend)
        convs = [m for m in mods if isinstance(m, nn.Conv2d)]
        for j, m in enumerate(convs):
            k = mods.index(m)
            pool_after = any(isinstance(mods[t], nn.MaxPool2d) for t in range(k + 1, min(k + 3, len(mods))))
            self.front.append(ConvSpec(j, m, m.in_channels, m.out_channels, 3, 1, first=(j == 0),
                                       pool_after=pool_after, w_index=pid[id(m.weight)], b_index=pid[id(m.bias)]))
        self.back: List[ConvSpec] = []
        for j, m in enumerate([m for m in model._modules["backend"] if isinstance(m, nn.Conv2d)]):
            self.back.append(ConvSpec(j, m, m.in_channels, m.out_channels, 3, m.dilation[0],
                                      w_index=pid[id(m.weight)], b_index=pid[id(m.bias)]))
        self.head = model.output_layer
        self.head_w_index, self.head_b_index = pid[id(self.head.weight)], pid[id(self.head.bias)]
        self.ctx1 = {s: getattr(model, f"conv{s}_1") for s in CONTEXT_SCALES}
        self.ctx2 = {s: getattr(model, f"conv{s}_2") for s in CONTEXT_SCALES}
        self.ctx1_index = {s: pid[id(self.ctx1[s].weight)] for s in CONTEXT_SCALES}
        self.ctx2_index = {s: pid[id(self.ctx2[s].weight)] for s in CONTEXT_SCALES}
        self.packs: Dict[int, tuple] = {}
        self._pack_version = None
        self._pack_desc = None          # device descriptor rows of the batched pack launch
        self._pack_desc_ptrs = None
        self._opt_key = None            # opt_prepare: the arena and parameter addresses its rows were built for,
        self._opt_desc = None           #   the device descriptor rows of the fused optimizer / swap launch
        self._opt_tiles = 0             #   and its grid width
        self.ws = None
        self.last_wvalid = None         # valid width of the last forward's b6 when it was width-padded
        self._ws_need = {}              # (n, h, w, dispatch config) -> weight-gradient workspace floats
        self._w1g_buf = None            # conv1_1 weight-gradient slabs of the fused conv1_2 data gradient
        self.stream_override = None
        self._side = None
        self.split = None               # SplitCapture while the stepper captures the two streams as two graphs

    def grad_ready_order(self) -> List[int]:
        """Parameter indices in the order backward_features produces them."""
        order = [self.head_w_index, self.head_b_index]
        for s in reversed(self.back):
            order += [s.w_index, s.b_index]
        order += [self.ctx2_index[sc] for sc in CONTEXT_SCALES]
        order += [self.ctx1_index[sc] for sc in CONTEXT_SCALES]
        for s in reversed(self.front):
            order += [s.w_index, s.b_index]
        return order

    # ----------------------------------------------------------- weights
    def _params(self):
        return self._plist

    def _weights_version(self):
        return tuple(p._version for p in self._params())

    def _alloc_packs(self, device):
        for s in self.front + self.back:
            w = s.module.weight
            if s.first:
                # k = tap*4 + c: the pack kernel writes only c < 3, tap < 9 -> pad must be zero
                fwd = torch.zeros(s.cout, 64, dtype=self.act, device=device)
                dgr = None
            else:
                fwd = torch.empty(s.cout, s.ksize * s.ksize * s.cin, dtype=self.act, device=device)
                dgr = torch.empty(s.cin, s.ksize * s.ksize * s.cout, dtype=self.act, device=device)
            self.packs[id(w)] = (fwd, dgr)
        # the four conv{S}_2 packs are items of one [4, 512, 512] buffer each (one batched launch per pass)
        self.ctx2_fwd = torch.empty(len(CONTEXT_SCALES), 512, 512, dtype=self.act, device=device)
        self.ctx2_dgr = torch.empty_like(self.ctx2_fwd)
        for i, sc in enumerate(CONTEXT_SCALES):
            self.packs[id(self.ctx2[sc].weight)] = (self.ctx2_fwd[i], self.ctx2_dgr[i])
        # the linearised context module's interleaved packs: W2cat[4c + si] = W2_S[c] and its transpose
        nsc = len(CONTEXT_SCALES)
        self.ctx2cat_fwd = torch.empty(nsc * 512, 512, dtype=self.act, device=device)
        self.ctx2cat_dgr = torch.empty(512, nsc * 512, dtype=self.act, device=device)

    def _pack_rows(self):
        """Descriptor rows of the packed layers (elementwise.hip pack_multi_kernel, kPackRow = 12 int64):
        {w, fwd, dgr, Co, Ci, taps, first, mode 0, fwd2, dgr2, si, n}; each conv{S}_2 row also fills its scale's
        rows of the interleaved linearised-context packs (fwd2 / dgr2 / si)."""
        rows = []
        for s in self.front + self.back:
            fwd, dgr = self.packs[id(s.module.weight)]
            rows.append([s.module.weight.data_ptr(), fwd.data_ptr(), dgr.data_ptr() if dgr is not None else 0,
                         s.cout, s.cin, s.ksize * s.ksize, int(s.first), 0, 0, 0, 0, s.module.weight.numel()])
        for si, sc in enumerate(CONTEXT_SCALES):
            w = self.ctx2[sc].weight
            fwd, dgr = self.packs[id(w)]
            rows.append([w.data_ptr(), fwd.data_ptr(), dgr.data_ptr(), 512, 512, 1, 0, 0,
                         self.ctx2cat_fwd.data_ptr(), self.ctx2cat_dgr.data_ptr(), si, w.numel()])
        return rows

    def _packed_ptrs(self):
        return tuple(s.module.weight.data_ptr() for s in self.front + self.back) + \
            tuple(self.ctx2[sc].weight.data_ptr() for sc in CONTEXT_SCALES)

    def refresh_packs(self, force: bool = False):
        """Re-pack the 16-bit weight copies from the fp32 masters (one launch for all layers)."""
        ver = self._weights_version()
        if not force and ver == self._pack_version and self.packs:
            return
        dev = self.head.weight.device
        if not self.packs:
            self._alloc_packs(dev)
        st = self._stream()
        # one launch for every layer (descriptor rows hold the fp32 master pointers, which the flat arena keeps
        # fixed; rebuilt if a weight tensor moved)
        if self._pack_desc is None or self._packed_ptrs() != self._pack_desc_ptrs:
            rows = self._pack_rows()
            self._pack_desc = torch.tensor(rows, dtype=torch.int64, device=dev)
            self._pack_desc_ptrs = self._packed_ptrs()
            self._pack_tiles = max(((r[3] + 31) // 32) * ((r[4] + 31) // 32) for r in rows)
        self.C.pack_multi(self._pack_desc.data_ptr(), self._pack_desc.shape[0], self._pack_tiles, self.dt, st)
        self._pack_version = ver

    def opt_step(self, data: torch.Tensor, grad: torch.Tensor, mom: torch.Tensor, lr: float, gscale: float,
                 optimizer: str = "sgd", momentum: float = 0.95, weight_decay: float = 0.0, betas=(0.9, 0.999),
                 eps: float = 1e-8, mom2: Optional[torch.Tensor] = None, step: Optional[torch.Tensor] = None,
                 flags: Optional[torch.Tensor] = None, lr_dev: Optional[torch.Tensor] = None,
                 gmul: Optional[torch.Tensor] = None, ema: Optional[torch.Tensor] = None,
                 ema_t: Optional[torch.Tensor] = None, ema_decay: float = 0.0, ema_warmup: bool = True):
        """The fused optimizer step (elementwise.hip pack_multi_kernel<DT, OPT, EMA>): the update over every parameter
        of the flat arena ``data`` (gradients / momentum in the same layout in ``grad`` / ``mom``) and the 16-bit packs
        written from the updated weights, in ONE launch: the packs do not re-read the 83 MB of fp32 masters.
        ``optimizer`` = "sgd" (torch.optim.SGD with momentum, bit for bit the sgd_momentum kernel, and coupled
        ``weight_decay``, its own instantiation when not 0), "adam" (torch.optim.Adam,
        coupled weight decay) or "adamw" (decoupled).  flags / lr_dev: the native step's device flag vector (a
        non-finite loss or gradient skips the step, weights and packs untouched) and learning rate.
        Adam: ``mom`` / ``mom2`` are the first / second moment arenas
        and ``step`` the int32 device count of applied steps, which a one-thread launch after the step advances
        unless the step was skipped through ``flags``.  ``gmul``: an fp32 device scalar the kernel multiplies into
        ``gscale`` (one fp32 product: the clip coefficient of ``grad_norm``).  ``ema``: an fp32 arena like ``data``
        holding the exponential moving average of the parameters, updated in the same launch from the masters as
        stored (e += w (p - e), w = 1 - min(ema_decay, (1 + n) / (10 + n)) with ``ema_warmup``, n = ``ema_t``, the
        int32 device count of applied updates, advanced with the step unless it was skipped)."""
        desc, rows, tiles, goff, boff, voff, eoff = self.opt_prepare(data, grad, mom, mom2, ema)
        if ema is not None:
            if ema_t is None or ema_t.dtype != torch.int32 or ema_t.device != data.device or ema_t.numel() < 1:
                raise ValueError("opt_step: ema_t must be an int32 tensor on the arena's device")
            if not 0.0 <= float(ema_decay) < 1.0:
                raise ValueError(f"opt_step: ema_decay must be in [0, 1), got {ema_decay!r}")
        if gmul is not None and not (gmul.dtype == torch.float32 and gmul.device == data.device and gmul.numel() >= 1):
            raise ValueError("opt_step: gmul must be an fp32 tensor on the arena's device")
        if optimizer not in ("sgd", "adam", "adamw"):
            raise ValueError(f"opt_step: unknown optimizer {optimizer!r}")
        adam = optimizer != "sgd"
        if adam:
            if mom2 is None or step is None:
                raise ValueError("opt_step: Adam needs the second-moment arena and the device step count")
            if step.dtype != torch.int32 or step.device != data.device or step.numel() < 1:
                raise ValueError("opt_step: step must be an int32 tensor on the arena's device")
        kind = 3 if adam else (2 if weight_decay != 0 else 1)
        self.C.opt_pack(desc, rows, tiles, kind, goff, boff, voff, float(lr), float(momentum), float(betas[0]),
                        float(betas[1]), float(eps), float(weight_decay), int(optimizer == "adamw"), float(gscale),
                        step.data_ptr() if adam else 0, flags.data_ptr() if flags is not None else 0,
                        lr_dev.data_ptr() if lr_dev is not None else 0, self.dt, self._stream(),
                        gmul.data_ptr() if gmul is not None else 0, eoff, float(ema_decay), int(bool(ema_warmup)),
                        ema_t.data_ptr() if ema is not None else 0)
        self._pack_version = self._weights_version()

    def swap_weights(self, data: torch.Tensor, ema: torch.Tensor):
        """Exchange the masters with the EMA arena in ONE launch over the optimizer's descriptor rows and write every
        16-bit pack from the values that land in the master slots.  The parameters are views of ``data``, so the model
        now holds (evaluates, saves) the other set of weights; no address changes, so captured graphs stay valid.  Two
        swaps in a row are the identity, packs included."""
        if self._opt_key is None or self._opt_key[0] != data.data_ptr():
            raise RuntimeError("swap_weights: call opt_prepare on this arena first")
        self.C.swap_pack(self._opt_desc.data_ptr(), self._opt_desc.shape[0], self._opt_tiles,
                         self._arena_off(data, ema, "EMA"), self.dt, self._stream())
        self._pack_version = self._weights_version()

    def norm_prepare(self, grad: torch.Tensor, slots: Sequence):
        """The gradient-norm pass's device table and scratch for this gradient arena (elementwise.hip
        grad_norm_partial_kernel / grad_norm_final_kernel); ``slots``: (element offset, element count) of every
        parameter in arena order.  Built once: call before a graph capture (the build copies to the device).
        Returns ``gn``, the fp32 result vector {global norm, clip coefficient, per-parameter norms in slot order}."""
        if grad.dtype != torch.float32 or not grad.is_contiguous():
            raise ValueError("norm_prepare: the gradient arena must be contiguous fp32")
        slots = [(int(o), int(n)) for o, n in slots]
        if not slots or any(o < 0 or n < 0 or o + n > grad.numel() for o, n in slots):
            raise ValueError("norm_prepare: every slot must lie inside the gradient arena")
        dev = grad.device
        chunk = self.C.grad_norm_chunk()
        self._norm_max = max(n for _, n in slots)
        self._norm_np = len(slots)
        self._norm_tab = torch.tensor(slots, dtype=torch.int64, device=dev)
        self._norm_part = torch.zeros(len(slots) * max(1, -(-self._norm_max // chunk)), dtype=torch.float64, device=dev)
        self._norm_grad = grad
        self.gn = torch.zeros(2 + len(slots), dtype=torch.float32, device=dev)
        return self.gn

    def grad_norm(self, gscale: float, max_norm: float, flags: Optional[torch.Tensor] = None):
        """Two launches over the prepared arena: gn[0] = gscale * ||g||, gn[1] = min(1, max_norm / (gn[0] + 1e-6))
        (``inf``: measure only, exactly 1), gn[2 + i] = gscale * ||g_i||.  A non-finite gradient gives coefficient 0
        and sets flags[2], which the optimizer kernels skip on."""
        self.C.grad_norm(self._norm_grad.data_ptr(), self._norm_tab.data_ptr(), self._norm_np, self._norm_max,
                         self._norm_part.data_ptr(), self.gn.data_ptr(), float(gscale), float(max_norm),
                         flags.data_ptr() + 8 if flags is not None else 0, self._stream())
        return self.gn

    @staticmethod
    def _arena_off(data: torch.Tensor, other: torch.Tensor, what: str) -> int:
        if other.shape != data.shape or other.dtype != torch.float32 or other.device != data.device or \
                not other.is_contiguous():
            raise ValueError(f"opt_step: the {what} arena must match the parameter arena")
        if (other.data_ptr() - data.data_ptr()) % data.element_size():
            raise ValueError("opt_step: arena offsets must be whole floats")
        off = (other.data_ptr() - data.data_ptr()) // data.element_size()
        if abs(off) < data.numel():
            raise ValueError(f"opt_step: the {what} arena overlaps the parameter arena")
        return off

    def opt_prepare(self, data: torch.Tensor, grad: torch.Tensor, mom: torch.Tensor,
                    mom2: Optional[torch.Tensor] = None, ema: Optional[torch.Tensor] = None):
        """The fused optimizer's launch arguments for these arenas: (descriptor rows' device pointer, row count, grid
        width, then the gradient / momentum / second-moment / EMA arena's offset from ``data`` in floats, 0 without
        one).  The parameters are validated and the rows built once per layout of the masters (call before a graph
        capture: the build copies the rows to the device): a repeated call compares the addresses of ``data`` and of
        every parameter, so a moved one is still noticed, and checks the four arenas against ``data``."""
        key = (data.data_ptr(), data.numel(), tuple(p.data_ptr() for p in self._plist))
        if key != self._opt_key:
            if not self.packs:
                self._alloc_packs(self.head.weight.device)
            base, end = key[0], key[0] + key[1] * data.element_size()
            for p in self._plist:
                if not (p.dtype == torch.float32 and p.is_contiguous() and base <= p.data_ptr() < end):
                    raise ValueError("opt_prepare: every parameter must be a contiguous fp32 view of the arena")
            rows = self._pack_rows()
            packed = {r[0] for r in rows}
            for p in self._plist:
                if p.data_ptr() not in packed:           # biases, head, conv{S}_1: no pack
                    rows.append([p.data_ptr(), 0, 0, 0, 0, 0, 0, -1, 0, 0, 0, p.numel()])
            if sorted(r[0] for r in rows) != sorted(key[2]):
                raise RuntimeError("opt_prepare: the descriptor rows do not cover every parameter exactly once")
            self._opt_desc = torch.tensor(rows, dtype=torch.int64, device=data.device)
            self._opt_tiles = max(((r[3] + 31) // 32) * ((r[4] + 31) // 32) if r[7] >= 0 else -(-r[11] // 4096)
                                  for r in rows)
            self._opt_key = key
        return (self._opt_desc.data_ptr(), self._opt_desc.shape[0], self._opt_tiles,
                self._arena_off(data, grad, "gradient"), self._arena_off(data, mom, "momentum"),
                self._arena_off(data, mom2, "second-moment") if mom2 is not None else 0,
                self._arena_off(data, ema, "EMA") if ema is not None else 0)

    def _stream(self):
        return self.stream_override if self.stream_override is not None else _ext.stream_ptr(self.head.weight.device)

    PAD_ALIGN = 64

    def padded_width(self, w: int, h: Optional[int] = None) -> int:
        """Row pitch the executor runs an input of width w (and height h, when given) at (see "Ragged widths"): w
        rounded up to a multiple of 64 when w is not one (dispatch pad_width, linearised context module), else w.
        An input of fewer than 24 rows is never padded: its 1/8-resolution map has fewer than 3 rows and runs the
        direct context module (ops.conv.ctx_linear_ok), which takes no padded map."""
        d = dispatch.current()
        if not d.pad_width or w % self.PAD_ALIGN == 0 or not d.ctx_linear or (h is not None and h < 24):
            return w
        wp = -(-w // self.PAD_ALIGN) * self.PAD_ALIGN
        return wp if wp // 8 >= 64 else w      # the linear context GEMM needs a 1/8-resolution pitch >= 64

    def workspace(self, n, h, w):
        """Size the shared wgrad slab workspace for an input of [n,3,h,w] (call before graph capture)."""
        if self.ws is None:
            self.ws = C.WgradWorkspace(self.head.weight.device)
        key = (n, h, w, dispatch.current())
        got = self._ws_need.get(key)
        if got is not None:                       # sized for this shape already (the planner is ~30 native calls)
            self.ws.reserve(got)
            if dispatch.current().w1g:
                self._w1g_slabs(self.head.weight.device)
            return self.ws
        need = 0
        hh, ww = h, self.padded_width(w, h)
        for s in self.front:
            _, _, _, nd = self.ws.plan(n * hh * ww, 4 if s.first else s.cin, s.cout, 3, s.first, 1, ww)
            need = max(need, nd)
            if s.pool_after:
                hh, ww = hh // 2, ww // 2
        for s in self.back:
            need = max(need, self.ws.plan(n * hh * ww, s.cin, s.cout, 3, False, s.dil, ww)[3])
        need = max(need, self.ws.plan(n * hh * ww, 512, 512, 1, False)[3])
        need = max(need, self.ws.plan(n * hh * ww, 512, 4 * 512, 1, False)[3])    # linearised context dW2cat
        need = max(need, max(C.wgrad_1x1_batched_plan(n * hh * ww, 4, 512, 512, ncu=c)[2] for c in (128, 192, 224, 256)))
        self._ws_need[key] = need
        self.ws.reserve(need)
        if dispatch.current().w1g:
            self._w1g_slabs(self.head.weight.device)
        return self.ws

    def _w1g_ok(self, x) -> bool:
        """conv1_1's weight gradient fused into conv1_2's data gradient (conv_dgrad_w1g; dispatch w1g = 0: separate
        weight-gradient launch on the side stream).  Measured 453.5 -> 456.7 img/s, peak HBM 8.75 -> 7.95 GB
        (profiles/r2/ab_w1g.txt)."""
        f0, f1 = self.front[0], self.front[1]
        return (dispatch.current().w1g and f0.first and f0.cout == 64 and f1.cin == 64
                and f1.cout == 64 and not f0.pool_after and x.dim() == 4 and x.shape[-1] == 64)

    def _w1g_slabs(self, device):
        if self._w1g_buf is None or self._w1g_buf[0].device != device:
            cap = C.w1g_slab_cap(device)
            self._w1g_buf = (torch.empty(cap, 36 * 64, dtype=torch.float32, device=device),
                             torch.empty(cap, 64, dtype=torch.float32, device=device))
        return self._w1g_buf

    # ----------------------------------------------------------- forward
    def _conv(self, s: ConvSpec, x, epi=C.EPI_BIAS_RELU, mask_bits_out=None, wvalid=None):
        fwd, _ = self.packs[id(s.module.weight)]
        return C.conv_igemm(x, fwd, s.module.bias.detach(), ksize=s.ksize, dil=s.dil, epi=epi, first=s.first,
                            mask_bits_out=mask_bits_out, wvalid=wvalid)

    def _sign_bits_out(self, s: ConvSpec, x):
        """uint8 sign-bit buffer [N,H,W,Cout/8] for this frontend conv's output when its forward can write them and the
        next layer's data gradient (or conv1_2's fused w1g kernel) reads them as its ReLU mask (dispatch sign_masks;
        conv_igemm.hip EPI_MASKB), else None."""
        if not dispatch.current().sign_masks or s.pool_after or s.idx + 1 >= len(self.front):
            return None
        t = self.front[s.idx + 1]
        n, h, w = x.shape[0], x.shape[1], x.shape[2]
        if s.first:
            ok = (t.idx == 1 and dispatch.current().w1g and s.cout == 64 and t.cin == 64 and t.cout == 64 and
                  x.shape[-1] == 4 and C.mask_bits_out_ok(4, 64, first=True))
        else:
            ok = C.mask_bits_out_ok(s.cin, s.cout) and C.mask_bits_ok(h, w, t.cout, t.cin, 1)
        if not ok:
            return None
        return torch.empty(n, h, w, s.cout // 8, dtype=torch.uint8, device=x.device)

    def _pool_fused(self, s: ConvSpec, x) -> bool:
        """The 2x2 max-pool after this conv runs in the conv's epilogue (LDS-DMA kernels; conv1_2: the halo
        kernel's epilogue through an LDS staging tile).  Dispatch pool_fwd_fused = 0: separate pool kernel."""
        return (s.pool_after and not s.first and s.dil == 1 and (s.cin != 64 or s.cout == 64)
                and dispatch.current().pool_fwd_fused and C.conv_pool_fwd_ok(x, s.cout, s.ksize))

    def _maxpool(self, x):
        """(pooled, max-pool codes): the codes replace the pool input in the saved state."""
        n, h, w, c = x.shape
        y = torch.empty(n, h // 2, w // 2, c, dtype=self.act, device=x.device)
        codes = torch.empty(n, h // 2, w // 2, c // 8, dtype=torch.int32, device=x.device)
        self.C.maxpool_fwd(x.data_ptr(), y.data_ptr(), n, h, w, c, self.dt, self._stream(), codes.data_ptr())
        return y, codes

    def _img(self, img):
        if img.dim() == 4 and img.shape[-1] == 4 and img.dtype in C.ACT_DTYPES:
            if img.dtype != self.act:
                raise ValueError(f"NHWC4 input is {img.dtype}, the executor computes in {self.act}")
            # already in the first layer's NHWC4 layout (ops/preprocess.py)
            if img.shape[1] % 8 or img.shape[2] % 8:
                raise ValueError("H, W must be multiples of 8")
            return img.contiguous()
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError("input must be [N,3,H,W]")
        n, _, h, w = img.shape
        if h % 8 or w % 8:
            raise ValueError(f"H, W must be multiples of 8 (got {h}x{w}); resize as CrowdDataset does")
        img = img.float().contiguous()
        x4 = torch.empty(n, h, w, 4, dtype=self.act, device=img.device)
        self.C.img_to_nhwc4(img.data_ptr(), x4.data_ptr(), n, h, w, self.dt, self._stream())
        return x4

    def _pad(self, x):
        """(x at the padded row pitch, valid width or None) for an NHWC4 input (see "Ragged widths")."""
        n, h, w, c = x.shape
        wp = self.padded_width(w, h)
        if wp == w:
            return x, None
        xp = torch.zeros(n, h, wp, c, dtype=x.dtype, device=x.device)
        xp[:, :, :w].copy_(x)
        return xp, w

    def forward_features(self, img, save: bool):
        """Runs everything up to the last backend ReLU. Returns (b6 [N,h,w,64], saved dict); for a width-padded
        input b6 is at the padded pitch and ``self.last_wvalid`` (and sv["wv8"]) is the valid width of b6."""
        self.refresh_packs()
        sv = {} if save else None
        x, wv = self._pad(self._img(img))
        acts = []   # conv inputs of the frontend
        pre_pool = {}
        mbits = {}  # frontend layer index -> sign bits of its output (the next layer's data-gradient ReLU mask)
        for s in self.front:
            acts.append(x)
            if self._pool_fused(s, x):
                # conv + ReLU + pool in one kernel; only the pooled map and the max-pool codes are written
                # (the full-resolution output is never stored: the backward needs the codes alone)
                fwd, _ = self.packs[id(s.module.weight)]
                _, x, codes = C.conv_pool_fwd(x, fwd, s.module.bias.detach(), ksize=s.ksize, dil=s.dil,
                                              keep_full=False, codes=save, wvalid=wv)
                if save:
                    pre_pool[s.idx] = codes
                wv = None if wv is None else wv // 2
                continue
            else:
                bits = self._sign_bits_out(s, x) if save else None
                y = self._conv(s, x, mask_bits_out=bits, wvalid=wv)
                if bits is not None:
                    mbits[s.idx] = bits
            if s.pool_after:
                x, codes = self._maxpool(y)
                pre_pool[s.idx] = codes
                wv = None if wv is None else wv // 2
            else:
                x = y
        fv = x
        cat, ctx_saved = self._context_fwd(fv, save, wv)
        x = cat
        back_in = []
        for s in self.back:
            back_in.append(x)
            x = self._conv(s, x, wvalid=wv)
        self.last_wvalid = wv
        if save:
            sv.update(front_in=acts, pre_pool=pre_pool, fv=fv, ctx=ctx_saved, back_in=back_in, b6=x, mbits=mbits,
                      wv8=wv)
        return x, sv

    def head_forward(self, b6, wvalid: Optional[int] = None):
        """Density map [N,1,h,w] of b6; a width-padded b6 (wvalid) gives the map at the valid width."""
        n, h, w, _ = b6.shape
        et = torch.empty(n, 1, h, w, dtype=torch.float32, device=b6.device)
        wv = C._wv(wvalid, w)
        self.C.head_fwd(b6.data_ptr(), self.head.weight.detach().data_ptr(), self.head.bias.detach().data_ptr(),
                        et.data_ptr(), n * h * w, self.dt, self._stream(), w if wv else 0, wv)
        return et[..., :wv].contiguous() if wv else et

    @torch.no_grad()
    def forward_eval(self, img):
        b6, _ = self.forward_features(img, save=False)
        return self.head_forward(b6, self.last_wvalid)

    # ----------------------------------------------------------- backward
    def backward_features(self, sv, d_b6: torch.Tensor, grads: Sequence[Optional[torch.Tensor]],
                          on_grad_ready: Optional[Callable[[List[int]], None]] = None, beta: float = 0.0,
                          scale: float = 1.0, dscale: Optional[torch.Tensor] = None):
        """d_b6: grad wrt the PRE-activation of the last backend conv (ReLU already applied).

        grads[i] is the fp32 output tensor for model.parameters()[i] (written, or
        accumulated when beta=1).  Entries for the head must already be filled.
        dscale: optional fp32 device scalar multiplied into every weight gradient
        (1 / loss scale when d_b6 carries a loss scale, fp16 step).
        (A data-gradient chain on a high-priority stream measured neutral: profiles/r4/ab_confirm.txt.)
        """
        ws = self.ws or self.workspace(*self._shape_from(sv))
        ready = on_grad_ready or (lambda idx: None)
        side = self._side_stream()
        hold = []          # operands of side-stream work, kept alive until the join below

        # the data-gradient epilogues also sum the bias gradient of the dY they write, so the weight-gradient
        # launch need not re-read dY for db (the bias column sums were ~1 ms/step of weight-gradient-stream
        # time).  Round 2 measured it negative (421-423 vs 427 img/s, profiles/r2/README.md); after the round-3
        # kernel changes it is ahead in every interleaved round (485.5-485.8 vs 483.3-485.1 img/s,
        # profiles/r3/ab_bias_fused.txt), so it is the default; dispatch bias_fused = 0 re-reads dY
        fuse_bias = bool(dispatch.current().bias_fused)

        def wg(dy, x, ksize, dil, first, wi, bi, bp=None):
            # bp: bias partials of dy summed by the data-gradient epilogue that wrote it (None: the weight-
            # gradient launch re-reads dy for the bias)
            def run():
                C.conv_wgrad(dy, x, grads[wi], grads[bi] if bi is not None else None, ksize=ksize, dil=dil,
                             first=first, ws=ws, beta=beta, scale=scale, dscale=dscale, bias_partials=bp)
                ready([wi] + ([bi] if bi is not None else []))
            # (one fork per layer: queuing every other layer's weight gradient for the next fork halved the forks
            # and their ~4.8 us compute-stream bubbles, but delayed the side stream: batch 8 neutral, batch 1 -0.8 %,
            # profiles/r6/ab_fork_pairs_negative.jsonl)
            self._on_side(side, run, hold, dy, x, *(() if bp is None else (bp,)))

        def dgrad(dy, dgr, dil, epi, mask, bits=None):
            """Data gradient; returns (dX, bias partials of dX or None).  bits: the mask as sign bits."""
            if fuse_bias:
                return C.conv_dgrad_with_bias(dy, dgr, ksize=3, dil=dil, epi=epi, mask=mask, mask_bits=bits)
            return C.conv_igemm(dy, dgr, None, ksize=3, dil=dil, epi=epi, mask=mask, mask_bits=bits), None
        mbits = sv.get("mbits") or {}

        # ---- backend, reverse
        dy, bp = d_b6, None
        for s in reversed(self.back):
            x = sv["back_in"][s.idx]
            wg(dy, x, 3, s.dil, False, s.w_index, s.b_index, bp)
            _, dgr = self.packs[id(s.module.weight)]
            if s.idx > 0:
                dy, bp = dgrad(dy, dgr, s.dil, C.EPI_MASK, x)
            else:
                dcat = C.conv_igemm(dy, dgr, None, ksize=3, dil=s.dil, epi=C.EPI_NONE)
        # ---- context module
        dy = self._context_bwd(sv["ctx"], sv["fv"], dcat, grads, ws, beta, scale, ready, dscale, side, hold)
        # ---- frontend, reverse
        bp = None
        for s in reversed(self.front):
            x = sv["front_in"][s.idx]
            wg(dy, x, 3, 1, s.first, s.w_index, s.b_index, bp)
            if s.idx == 0:
                break
            _, dgr = self.packs[id(s.module.weight)]
            prev = self.front[s.idx - 1]
            if s.idx == 1 and prev.first and self._w1g_ok(x):
                # conv1_2's data gradient with conv1_1's weight gradient fused (compute stream): conv1_1's dY is
                # consumed tile by tile inside the kernel, never written to or re-read from memory
                img = sv["front_in"][0]
                sl, bsl = self._w1g_slabs(x.device)
                C.conv_dgrad_w1g(dy, dgr, x, img, grads[prev.w_index], grads[prev.b_index], slabs=sl, bslabs=bsl,
                                 beta=beta, scale=scale, dscale=dscale, mask_bits=mbits.get(prev.idx))
                if side is not None:
                    # join before marking ready: the bucket holding conv1_1 also holds side-stream gradients, and a
                    # transport that orders its all-reduce after the marking stream must see them too
                    self._join(side)
                ready([prev.w_index, prev.b_index])
                break
            if prev.pool_after:
                # data gradient at the pooled resolution, scattered through the max-pool backward
                # (+ ReLU mask of the pool input) in the conv epilogue: the pooled gradient never
                # round-trips through memory
                codes = sv["pre_pool"][prev.idx]
                # (conv2_1's data gradient / conv1_2's weight gradient in image halves measured -0.5 %:
                # profiles/r4/ab_tail_split.txt)
                if dispatch.current().poolbwd_fused:
                    dy, bp = dgrad(dy, dgr, 1, C.EPI_POOLBWD, codes)
                else:
                    dp = C.conv_igemm(dy, dgr, None, ksize=3, dil=1, epi=C.EPI_NONE)
                    dy, bp = C.maxpool_bwd_codes(codes, dp), None
            else:
                dy, bp = dgrad(dy, dgr, 1, C.EPI_MASK, x, mbits.get(prev.idx))
        if side is not None:
            self._join(side)                                             # join: every gradient written
        hold.clear()

    def _side_stream(self):
        """Weight gradients run on a second stream, concurrently with the data-gradient chain (they only
        need the layer's dY and input).  The memory-bound slab reductions / bias column sums and the
        partial last waves of one chain fill the CUs the other leaves idle.  Fork/join through stream
        waits, so the pattern is hipGraph-capturable; dispatch wgrad_stream = 0 runs everything in order.  (A
        high-priority side stream measured negative, profiles/r2/ab_side_priority_negative.txt.)"""
        if not dispatch.current().wgrad_stream or self.stream_override is not None:
            return None
        dev = self.head.weight.device
        if self._side is None or self._side.device != dev:
            self._side = _ext.own_stream(dev)         # (not a torch pool stream: _ext.own_stream)
        return self._side

    def _on_side(self, side, fn, hold, *keep):
        """Run ``fn``'s native launches on the side stream after everything issued so far on the compute stream
        (fork by one native event record / wait; the launches reach the side stream through _ext.launch_on, torch's
        current stream is left alone: ~20 us less host time per fork than torch.cuda.stream + wait_stream)."""
        if side is None:
            fn()
            return
        sp = side.cuda_stream
        if self.split is not None:
            self.split.fork(sp, self._stream())                           # external record / wait nodes
        else:
            self.C.stream_wait(sp, self._stream())                         # fork after the producers
        with _ext.launch_on(sp):
            fn()
        hold.extend(keep)

    def _join(self, side):
        """The compute stream waits for everything issued on the side stream (split capture: the side graph records
        its end; the stepper's second compute graph waits for it)."""
        if self.split is not None:
            self.split.side_end(side.cuda_stream)
        else:
            self.C.stream_wait(self._stream(), side.cuda_stream)

    @staticmethod
    def _shape_from(sv):
        x0 = sv["front_in"][0]
        return x0.shape[0], x0.shape[1], x0.shape[2]

    @staticmethod
    def input_hw(img):
        """(N, H, W) of an NCHW image batch or an NHWC4 prepacked batch."""
        if img.dim() == 4 and img.shape[-1] == 4 and img.dtype in C.ACT_DTYPES:
            return img.shape[0], img.shape[1], img.shape[2]
        return img.shape[0], img.shape[2], img.shape[3]

    # ----------------------------------------------------------- training head
    def head_train(self, b6, gt, grads, gscale: float = 1.0, beta: float = 0.0,
                   lscale: Optional[torch.Tensor] = None, flags: Optional[torch.Tensor] = None,
                   wvalid: Optional[int] = None):
        """Fused: et, MSE(sum) loss, d(et), d(b6 pre-act) (ReLU-masked), head grads. Returns (loss, et, d_b6).
        lscale: optional fp32 device scalar (loss scale) applied to d_b6 only; head grads stay unscaled.
        flags: optional fp32 device vector; the loss is written to flags[1] and its non-finite flag
        (1.0 / 0.0) to flags[0] by the same reduction kernel (the returned loss is then flags[1:2]).
        wvalid: b6 is width-padded with this valid width (default: the last forward's); gt is at the valid width,
        the padding columns add nothing to the loss or the gradients and et is returned at the valid width.
        gt [n,2,h,wg] fp32: channel 0 the ground truth, channel 1 a per-pixel loss weight m (loss = sum m (et-gt)^2,
        head_train_kernel<DT, true>); et stays unweighted.  A [n,1,h,wg] gt issues exactly the unweighted launch."""
        n, h, w, c = b6.shape
        wvalid = self.last_wvalid if wvalid is None else wvalid
        wv = C._wv(wvalid, w)
        wg = wv or w
        wt = None
        if tuple(gt.shape) == (n, 2, h, wg):
            # ground truth and per-pixel loss weight in one tensor (README, "ROI masks"): two contiguous planes
            if gt.dtype != torch.float32:
                raise ValueError(f"a 2-channel gt (ground truth, loss weight) must be fp32, got {gt.dtype}")
            gt, wt = gt[:, 0:1].contiguous(), gt[:, 1:2].contiguous()
        elif tuple(gt.shape) != (n, 1, h, wg):
            raise ValueError(f"gt shape {tuple(gt.shape)} != {(n, 1, h, wg)} (or {(n, 2, h, wg)} with a loss weight)")
        gt = gt.float().contiguous()
        if wv:
            gp = torch.zeros(n, 1, h, w, dtype=torch.float32, device=gt.device)
            gp[..., :wv].copy_(gt)
            gt = gp
            if wt is not None:
                wp = torch.zeros(n, 1, h, w, dtype=torch.float32, device=gt.device)
                wp[..., :wv].copy_(wt)
                wt = wp
        P = n * h * w
        et = torch.empty(n, 1, h, w, dtype=torch.float32, device=b6.device)
        d_b6 = torch.empty_like(b6)
        nblk = max(1, min(1024, (P * 8 + 255) // 256))
        part = torch.empty(nblk, 66, dtype=torch.float32, device=b6.device)
        if flags is not None:
            if not (flags.dtype == torch.float32 and flags.is_contiguous() and flags.numel() >= 2):
                raise ValueError("flags must be a contiguous fp32 vector of >= 2 elements")
            loss, nf = flags[1:2], flags.data_ptr()
        else:
            loss, nf = torch.empty(1, dtype=torch.float32, device=b6.device), 0
        self.C.head_train(b6.data_ptr(), self.head.weight.detach().data_ptr(), self.head.bias.detach().data_ptr(),
                          gt.data_ptr(), et.data_ptr(), d_b6.data_ptr(), part.data_ptr(), nblk,
                          grads[self.head_w_index].data_ptr(), grads[self.head_b_index].data_ptr(), loss.data_ptr(),
                          P, float(gscale), float(beta), lscale.data_ptr() if lscale is not None else 0, nf, self.dt,
                          self._stream(), w if wv else 0, wv, *(() if wt is None else (wt.data_ptr(),)))
        return loss, (et[..., :wv] if wv else et), d_b6

    # ----------------------------------------------------------- autograd entry
    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        if not torch.is_grad_enabled() or not any(p.requires_grad for p in self._params()):
            return self.forward_eval(img)
        return _CANNetFn.apply(img, self, *self._params())


class _CANNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, ex: CANNetExecutor, *params):
        b6, sv = ex.forward_features(img, save=True)
        et = ex.head_forward(b6, sv["wv8"])
        ctx.ex = ex
        ctx.sv = sv
        ctx.b6 = b6
        return et

    @staticmethod
    def backward(ctx, g_et):
        ex: CANNetExecutor = ctx.ex
        params = ex._params()
        grads = [torch.empty_like(p, dtype=torch.float32) for p in params]
        b6 = ctx.b6
        n, h, w, c = b6.shape
        g = g_et.float()
        wv = ctx.sv["wv8"]
        if wv is not None:                 # width-padded b6: no gradient at the padding columns
            gp = torch.zeros(n, 1, h, w, dtype=torch.float32, device=g.device)
            gp[..., :wv].copy_(g)
            g = gp
        g = g.reshape(n, h, w, 1)
        b6f = b6.float()
        hw = ex.head.weight.detach().view(1, c)
        d_b6 = (g * hw * (b6f > 0)).to(ex.act).contiguous()
        grads[ex.head_w_index].copy_((g * b6f).sum(dim=(0, 1, 2)).view_as(params[ex.head_w_index]))
        grads[ex.head_b_index].copy_(g.sum().view(1))
        ex.workspace(*CANNetExecutor._shape_from(ctx.sv))
        ex.backward_features(ctx.sv, d_b6, grads)
        ctx.sv = None
        return (None, None) + tuple(gr.to(p.dtype) for gr, p in zip(grads, params))
