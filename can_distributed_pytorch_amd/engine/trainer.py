"""Training-step engines shared by train.py and bench.py.

Two implementations of ONE training step (zero_grad -> forward -> MSE(sum)
-> backward + gradient all-reduce -> optimizer: SGD(momentum 0.95) by default, Adam / AdamW), the reference's
step (utils/train_eval_utils.py:28-52):

* ``TorchStepper`` — the stock PyTorch-ROCm reference stack: nn.Conv2d
  (MIOpen), ATen elementwise, torch DDP (RCCL), torch.optim.SGD.  Used as the
  "reference stack on MI355X" baseline and as the CPU/gloo path.
* ``NativeStepper`` — this framework: the native executor (HIP MFMA kernels,
  NHWC bf16, fused context module), the C++/RCCL bucketed reducer overlapped
  with backward on a side stream, fused multi-tensor SGD over the flat fp32
  master arena that also refreshes the bf16 packed weights, and (optionally)
  the whole step captured once into a hipGraph and replayed.
"""
from __future__ import annotations

import contextlib
from typing import Optional

import torch
import torch.distributed as dist

from ..models.cannet import CANNet
from .metrics import weighted_sq_loss


OPTIMIZERS = ("sgd", "adam", "adamw")


def _check_window(accum_steps, clip_grad_norm):
    if int(accum_steps) != accum_steps or accum_steps < 1:
        raise ValueError(f"accum_steps must be an integer >= 1, got {accum_steps!r}")
    if not clip_grad_norm >= 0:
        raise ValueError(f"clip_grad_norm must be >= 0 (0 = off, inf = measure only), got {clip_grad_norm!r}")


def check_ema_decay(d):
    if not 0.0 <= d < 1.0:
        raise ValueError(f"ema_decay must be in [0, 1) (0 = off), got {d!r}")


def ema_decay_at(n: int, decay: float, warmup: bool = True) -> float:
    """d_n of the n-th (0-based) EMA update, in Python doubles: min(decay, (1 + n) / (10 + n)) with warm-up."""
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


class ParamEma:
    """EMA of the parameters for the steppers whose optimizer runs in torch ops: per-parameter fp32 copies, updated
    after every applied optimizer step by e += w (p - e), w = float32(1 - d_n) (engine/native.py has the semantics and
    the fused kernel), and exchanged with the parameters' ``.data`` by ``ema_weights()``.  BatchNorm buffers are not
    averaged.  No communication: the average is a deterministic function of replicated weights."""

    def _ema_init(self, ema_decay: float, ema_warmup: bool):
        check_ema_decay(ema_decay)
        self.ema_decay = float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema_steps = 0
        self._ema = None
        self._ema_in = False

    def _ema_params(self):
        return list(self.model.parameters())

    def ema_start(self):
        """(Re)start the average from the current weights at n = 0 (call once the weights are final)."""
        if self.ema_decay > 0:
            self._ema = [p.detach().clone().float() for p in self._ema_params()]
            self.ema_steps = 0

    def ema_update(self):
        """One EMA update (after an applied optimizer step)."""
        if self._ema is None:
            return
        d = ema_decay_at(self.ema_steps, self.ema_decay, self.ema_warmup)
        w = float(torch.tensor(1.0 - d, dtype=torch.float64).float())
        with torch.no_grad():
            for e, p in zip(self._ema, self._ema_params()):
                e.add_(p.detach().float() - e, alpha=w)
        self.ema_steps += 1

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model holds the EMA weights (``.data`` exchanged); the exit restores the raw weights,
        bit for bit.  Raises inside an open accumulation window and when EMA is off."""
        if self._ema is None:
            raise RuntimeError("ema_weights(): EMA is off (ema_decay = 0)")
        if self._micro != 0:
            raise RuntimeError("ema_weights(): an accumulation window is open; call flush() first")
        if self._ema_in:
            raise RuntimeError("ema_weights() does not nest")
        ps = self._ema_params()

        def swap():
            for i, p in enumerate(ps):
                raw = p.data
                p.data = self._ema[i].to(raw.dtype)
                self._ema[i] = raw
        swap()
        self._ema_in = True
        try:
            yield self.model
        finally:
            # back: the raw tensors return to the parameters untouched; the average was not changed inside
            for i, p in enumerate(ps):
                raw, avg = self._ema[i], p.data
                p.data = raw
                self._ema[i] = avg.float()
            self._ema_in = False

    def ema_state(self) -> Optional[dict]:
        if self._ema is None:
            return None
        names = [n for n, _ in self.model.named_parameters()]
        src = [p.data for p in self._ema_params()] if self._ema_in else self._ema
        return {"ema": {n: e.detach().float().clone() for n, e in zip(names, src)}, "steps": int(self.ema_steps)}

    def load_ema_state(self, ema: Optional[dict], steps: int = 0) -> bool:
        """Restore the average from a name-keyed dict (any stepper's ``ema_state()["ema"]``); None: restart it from
        the current weights at n = 0.  Returns whether a saved average was loaded."""
        if self.ema_decay <= 0:
            return False
        if not ema:
            self.ema_start()
            return False
        self._ema = [ema[n].detach().to(p.device).float().clone().view_as(p)
                     for n, p in self.model.named_parameters()]
        self.ema_steps = int(steps)
        return True


def make_torch_optimizer(params, optimizer="sgd", lr=1e-7, momentum=0.95, weight_decay=0.0, betas=(0.9, 0.999),
                         eps=1e-8):
    """torch.optim.SGD / Adam / AdamW from the steppers' common optimizer arguments."""
    if optimizer == "sgd":
        return torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay)
    if optimizer == "adam":
        return torch.optim.Adam(params, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
    if optimizer == "adamw":
        return torch.optim.AdamW(params, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
    raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")


class TorchStepper(ParamEma):
    exec_backend = "torch"

    def __init__(self, device, dtype="fp32", world=1, lr=1e-7, momentum=0.95, channels_last=None, model=None,
                 bucket_mb: float = 25.0, optimizer="sgd", weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8,
                 accum_steps: int = 1, clip_grad_norm: float = 0.0, ema_decay: float = 0.0, ema_warmup: bool = True):
        _check_window(accum_steps, clip_grad_norm)
        self._ema_init(ema_decay, ema_warmup)
        # gradient accumulation / global-norm clipping, the stock way: zero_grad at a window's start, DDP no_sync()
        # on its non-closing micro-steps, torch.nn.utils.clip_grad_norm_ ahead of the optimizer (engine/native.py has
        # the semantics: the sum-reduced loss needs no 1/k, lr is not rescaled)
        self.accum_steps = int(accum_steps)
        self.clip_grad_norm = float(clip_grad_norm)
        self._micro = 0
        self._acc = None
        self._grad_norm = None
        self.device = torch.device(device)
        self.model = (model or CANNet(backend=self.exec_backend)).to(self.device)
        self.model.exec_backend = self.exec_backend
        self.dtype = dtype
        self.channels_last = (dtype != "fp32") if channels_last is None else channels_last
        if self.channels_last:
            self.model = self.model.to(memory_format=torch.channels_last)
        self.net = self.model
        if world > 1:
            dev_ids = [self.device.index] if self.device.type == "cuda" else None
            self.net = torch.nn.parallel.DistributedDataParallel(self.model, device_ids=dev_ids,
                                                                 bucket_cap_mb=bucket_mb)
        self.optimizer = optimizer
        self.opt = make_torch_optimizer([p for p in self.model.parameters() if p.requires_grad], optimizer,
                                        lr=lr * world, momentum=momentum, weight_decay=weight_decay, betas=betas,
                                        eps=eps)
        self.crit = weighted_sq_loss                  # MSELoss(sum); a 2-channel gt carries a loss weight
        self._loss = None
        self.autocast = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(dtype)
        self.scaler = torch.amp.GradScaler("cuda") if dtype == "fp16" else None
        self.ema_start()                # (world > 1: DDP's constructor has broadcast rank 0's weights)

    def step(self, img, gt):
        """One micro-step; returns the window's loss on the call that closes it (accum_steps = 1: every call), else
        None."""
        closing = self._micro + 1 >= self.accum_steps
        if self._micro == 0:
            self.opt.zero_grad(set_to_none=True)
        if self.channels_last:
            img = img.contiguous(memory_format=torch.channels_last)
        sync = contextlib.nullcontext() if closing or self.net is self.model else self.net.no_sync()
        with sync:
            if self.autocast is not None:
                with torch.autocast(self.device.type, dtype=self.autocast):
                    et = self.net(img)
                loss = self.crit(et.float(), gt)
            else:
                et = self.net(img)
                loss = self.crit(et, gt)
            if self.scaler is not None:
                self.scaler.scale(loss).backward()
            else:
                loss.backward()
        self._acc = loss.detach() if self._micro == 0 else self._acc + loss.detach()
        self._micro += 1
        if not closing:
            return None
        return self._finish_window()

    def _finish_window(self):
        if self.clip_grad_norm > 0:
            if self.scaler is not None:
                self.scaler.unscale_(self.opt)
            self._grad_norm = torch.nn.utils.clip_grad_norm_(
                [p for p in self.model.parameters() if p.grad is not None], self.clip_grad_norm)
        if self.scaler is not None:
            before = self.scaler.get_scale() if self._ema is not None else None
            self.scaler.step(self.opt)
            self.scaler.update()
            if before is None or self.scaler.get_scale() >= before:      # (a backed-off scale: the step was skipped)
                self.ema_update()
        else:
            self.opt.step()
            self.ema_update()
        self._micro = 0
        self._loss = self._acc
        return self._loss

    def flush(self):
        """Close an open window now (end of an epoch); None when no window is open.  (World > 1: the window's earlier
        micro-steps ran under no_sync(), so call it only where every rank's window closes through step().)"""
        if self._micro == 0:
            return None
        return self._finish_window()

    def grad_norm(self) -> Optional[float]:
        return None if self._grad_norm is None else float(self._grad_norm)

    def last_loss(self) -> Optional[float]:
        return None if self._loss is None else float(self._loss)


class Fp32Stepper(TorchStepper):
    """Approximately-fp32 training numerics (the reference trains fp32, train.py:126) on the native kernels: every
    convolution — forward, data and weight gradient — runs as split-bf16 GEMMs on the MFMA conv kernels with fp32
    accumulation (ops/fp32.py: ~2^-16 relative error per product, not bitwise fp32); ReLU / pooling / the context module's elementwise math, the loss, DDP and SGD
    are the fp32 ATen / torch.distributed ones of TorchStepper."""
    exec_backend = "hip_fp32"

    def __init__(self, device, dtype="fp32", **kw):
        if dtype != "fp32":
            raise ValueError("Fp32Stepper is the fp32 step")
        super().__init__(device, dtype="fp32", channels_last=False, **kw)


class ArenaStepper(ParamEma):
    """This framework's data-parallel engine on the plain-ATen CANNet: the CPU / gloo rehearsal of the native step's
    distributed path (engine/native.py), used by ``bench.py --device cpu`` and the multi-process CPU tests.

    Same structure as the native step: fp32 parameters and gradients in one flat arena laid out in gradient-ready
    order (utils/flat.py), the bucketed reducer (parallel/reducer.py) driven by post-accumulate-grad hooks so
    buckets are all-reduced while autograd still runs, the loss and its non-finite flag in one 2-element collective,
    1/world folded into the SGD update (momentum 0.95, train.py:63,126 of the reference), the update skipped on a
    non-finite loss on every rank alike, and the init-time parameter sync as one broadcast of the arena."""
    exec_backend = "torch"

    def __init__(self, device="cpu", world=1, lr=1e-7, momentum=0.95, model=None, bucket_mb: float = 25.0,
                 optimizer="sgd", weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, accum_steps: int = 1,
                 clip_grad_norm: float = 0.0, ema_decay: float = 0.0, ema_warmup: bool = True):
        from ..models.cannet import grad_ready_order
        _check_window(accum_steps, clip_grad_norm)
        self._ema_init(ema_decay, ema_warmup)
        self.accum_steps = int(accum_steps)
        self.clip_grad_norm = float(clip_grad_norm)
        self._micro = 0
        self._acc = None
        self._gn = None                                      # (global norm, clip coefficient) of the last window
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")
        self.optimizer = optimizer
        self.weight_decay = float(weight_decay)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        from ..parallel.reducer import BucketedReducer
        from ..utils.flat import FlatArena
        self.device = torch.device(device)
        self.model = (model or CANNet(backend=self.exec_backend)).to(self.device)
        self.model.exec_backend = self.exec_backend
        self.world = world
        self.lr = lr * world                       # train.py:25 linear scaling
        self.momentum = momentum
        self.params = list(self.model.parameters())
        order = grad_ready_order(self.model)
        self.arena = FlatArena(self.params, self.device, order=order)
        self.mom = torch.zeros_like(self.arena.data)          # SGD momentum / Adam first moment
        self.mom2 = torch.zeros_like(self.arena.data) if optimizer != "sgd" else None
        self.opt_steps = 0                                    # applied Adam steps (the bias correction's t)
        self.reducer = BucketedReducer(self.arena, order, bucket_mb=bucket_mb, transport="torch")
        self.reducer.attach_hooks()
        self.flags = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.crit = weighted_sq_loss                  # MSELoss(sum); a 2-channel gt carries a loss weight
        self.comm_timing = False
        self._timings = []
        self._loss = None
        if world > 1:
            self.reducer.broadcast_arena(0)
        self.ema_start()

    def step(self, img, gt):
        """One micro-step (the native step's window: engine/native.py): the arena is zeroed at a window's start only,
        the reducer is paused on non-closing micro-steps (their autograd hooks launch nothing), and the closing one
        all-reduces the accumulated gradient once.  Returns the window's loss on the closing call, else None."""
        red = self.reducer
        closing = self._micro + 1 >= self.accum_steps
        red.set_timing(self.comm_timing)
        if self._micro == 0:
            self.arena.grad.zero_()
        self.arena.attach_grads()                  # autograd accumulates into the arena views in place
        red.paused = not closing
        if closing:
            red.begin()
        et = self.model(img.to(self.device))
        loss = self.crit(et, gt.to(self.device))
        loss.backward()
        self._acc = loss.detach() if self._micro == 0 else self._acc + loss.detach()
        self._micro += 1
        if not closing:
            return None
        return self._finish_window()

    def _finish_window(self):
        red = self.reducer
        red.finish()
        if self.comm_timing:
            self._timings.append(red.timings())
        with torch.no_grad():
            self.flags[0] = 0.0 if bool(torch.isfinite(self._acc)) else 1.0
            self.flags[1] = self._acc
            red.allreduce_scalars(self.flags)
            if self.flags[0] == 0 and self._update() is not False:
                self.ema_update()
        self._micro = 0
        self._loss = self.flags[1:2] / self.world
        return self._loss

    def flush(self):
        """Close an open window now (reducer begin / every parameter ready / finish, then the tail); None when no
        window is open."""
        if self._micro == 0:
            return None
        red = self.reducer
        red.paused = False
        red.begin()
        red.mark_ready(list(self.arena.order))
        return self._finish_window()

    def _clip(self) -> float:
        """1 / world times the native norm kernel's coefficient min(1, max_norm / (||g / W|| + 1e-6)) in torch ops;
        a non-finite norm skips the update (returns None), as the kernel's flags[2]."""
        gs = 1.0 / self.world
        if self.clip_grad_norm <= 0:
            return gs
        norm = (self.arena.grad.double().pow(2).sum().sqrt() * gs).float()
        if not bool(torch.isfinite(norm)):
            self._gn = (float(norm), 0.0)
            return None
        coef = torch.clamp(self.clip_grad_norm / (norm + 1e-6), max=1.0)
        self._gn = (float(norm), float(coef))
        return float(torch.tensor(gs, dtype=torch.float32) * coef)

    def grad_norm(self) -> Optional[float]:
        return None if self._gn is None else self._gn[0]

    def clip_coef(self) -> Optional[float]:
        return None if self._gn is None else self._gn[1]

    def _update(self):
        """The native step's three optimizers (elementwise.hip) in torch ops over the arena."""
        p, g, wd = self.arena.data, self.arena.grad, self.weight_decay
        gs = self._clip()
        if gs is None:
            return False                                     # skipped (non-finite norm): no EMA update either
        if self.optimizer == "sgd":
            # buf = m * buf + g / W (+ wd * p) ; p -= lr * buf   (torch.optim.SGD semantics, zero-initialised buffer)
            if wd != 0:
                g = (g * gs).add_(p, alpha=wd)
                self.mom.mul_(self.momentum).add_(g)
            else:
                self.mom.mul_(self.momentum).add_(g, alpha=gs)
            p.add_(self.mom, alpha=-self.lr)
            return
        # torch.optim.Adam / AdamW (no amsgrad), in torch's order of operations
        b1, b2 = self.betas
        g = g * gs
        if self.optimizer == "adamw":
            p.mul_(1.0 - self.lr * wd)
        elif wd != 0:
            g = g.add(p, alpha=wd)
        self.opt_steps += 1
        t = self.opt_steps
        self.mom.lerp_(g, 1.0 - b1)
        self.mom2.mul_(b2).addcmul_(g, g, value=1.0 - b2)
        denom = (self.mom2.sqrt() / (1.0 - b2 ** t) ** 0.5).add_(self.eps)
        p.addcdiv_(self.mom, denom, value=-self.lr / (1.0 - b1 ** t))

    def comm_report(self, reset: bool = True) -> Optional[dict]:
        """The last timed step's per-bucket all-reduce report (BucketedReducer.timings)."""
        t = [x for x in self._timings if x is not None]
        if reset:
            self._timings = []
        return t[-1] if t else None

    def last_loss(self) -> Optional[float]:
        return None if self._loss is None else float(self._loss.reshape(-1)[0])


def build_trainer(impl="hip", dtype="bf16", device="cuda", world=1, lr=1e-7, batch=8,
                  height=768, width=1024, graph=True, model=None, bucket_mb: float = 25.0,
                  reducer_transport: Optional[str] = None, comm_ctas: Optional[int] = None,
                  graph_bind_inputs: bool = False, graph_max_shapes: int = 8, optimizer: str = "sgd",
                  momentum: float = 0.95, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                  accum_steps: int = 1, clip_grad_norm: float = 0.0, ema_decay: float = 0.0,
                  ema_warmup: bool = True):
    opt = dict(optimizer=optimizer, momentum=momentum, weight_decay=weight_decay, betas=betas, eps=eps,
               accum_steps=accum_steps, clip_grad_norm=clip_grad_norm, ema_decay=ema_decay, ema_warmup=ema_warmup)
    if impl == "arena":
        return ArenaStepper(device, world=world, lr=lr, model=model, bucket_mb=bucket_mb, **opt)
    if impl == "torch":
        return TorchStepper(device, dtype=dtype, world=world, lr=lr, model=model, bucket_mb=bucket_mb, **opt)
    if dtype == "fp32":
        return Fp32Stepper(device, world=world, lr=lr, model=model, bucket_mb=bucket_mb, **opt)
    from .native import NativeStepper
    return NativeStepper(device, dtype=dtype, world=world, lr=lr, batch=batch, height=height,
                         width=width, graph=graph, model=model, bucket_mb=bucket_mb,
                         reducer_transport=reducer_transport, comm_ctas=comm_ctas,
                         graph_bind_inputs=graph_bind_inputs, graph_max_shapes=graph_max_shapes, **opt)
