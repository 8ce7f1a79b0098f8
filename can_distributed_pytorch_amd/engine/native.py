"""The native training step (this framework's hot path).

One step = the reference's step (utils/train_eval_utils.py:28-52):
zero_grad -> forward -> MSE(sum) -> backward (+ DDP all-reduce) -> SGD,
re-designed for MI355X:

* forward/backward: the static executor over gfx950 MFMA kernels
  (ops/executor.py), NHWC bf16 activations, fused head + loss + head-backward;
* gradients are written straight into a flat fp32 arena (utils/flat.py); each
  finished layer is handed to the bucketed reducer (parallel/reducer.py),
  which all-reduces full buckets over RCCL on a side stream while the
  remaining layers of the backward still run;
* the loss and its non-finite flag are written by the fused head's reduction
  kernel straight into a device flag vector, and travel in one 8-byte
  collective; averaging by 1/world is folded into the fused SGD kernel, which
  also skips the update on a non-finite loss and latches a sticky flag the
  host polls at its logging cadence (the reference's sys.exit guard,
  utils/train_eval_utils.py:48-50, made device-side and graph-safe);
* the learning rate lives in a device scalar read by the SGD kernel, so a
  captured step follows an lr schedule;
* roctx ranges (utils/profiling.trace_range, CANNET_ROCTX=1) mark the
  forward / backward / all-reduce / optimizer phases; ``comm_timing`` records
  hipEvents around the post-backward all-reduce join (exposed comm time);
* the optimizer update and the 16-bit weight packs are ONE kernel (executor.opt_step): the packs are written from the
  updated weights in registers, the 83 MB of fp32 masters are not re-read;
* with ``graph=True`` the whole step (for a fixed input shape) is captured
  once and replayed: one graph launch per stream per step instead of ~90 kernel
  launches.  SplitCapture: the compute stream, the weight-gradient stream and
  the native reducer's comm stream as separate chains joined by event nodes,
  each replayed on its own stream like the eager step (a torch-transport
  reducer falls back to one torch.cuda.CUDAGraph).  Stream priorities of a
  captured step:
  every stream the capture forks onto (the weight-gradient side stream and
  the RCCL reducer's comm stream) is at NORMAL priority — the reducer is built
  with ``comm_priority=0`` when ``graph=True`` (eager steps keep the comm stream
  at the highest priority).  Graph nodes carry no priority, and ending a
  capture that forked onto a high-priority stream crashed the ROCm 7.2 runtime
  (tests/test_gpu_executor.py covers a capture whose comm stream runs a kernel);
* ``dtype="fp16"`` runs the same kernels on fp16 activations / weight packs
  (v_mfma_f32_16x16x32_f16) with dynamic loss scaling kept on the device
  (graph-safe): the scale multiplies d(b6) inside the fused head, 1/scale is
  folded into every weight-gradient reduction, a gradient-overflow check
  after the all-reduce makes the fused SGD skip the step, and a one-thread
  kernel backs the scale off / grows it (GradScaler semantics: x0.5 on
  overflow, x2 after ``scale_interval`` clean steps).
* ``accum_steps=k`` makes k micro-steps one optimizer step on the SUM of their gradients (the sum-reduced loss needs
  no 1/k; lr is NOT rescaled by k): the opening micro-step overwrites the gradient arena (beta 0), later ones add to
  it (beta 1), and only the closing one runs the reducer, the loss all-reduce, the optimizer and the loss-scale
  update; ``clip_grad_norm=m`` adds a two-launch fixed-order norm pass over the accumulated, all-reduced arena whose
  clip coefficient the optimizer kernel reads from the device (``_step_tail``, README "Gradient accumulation and
  clipping").  With the defaults the step issues exactly the launches it issued before.
* ``ema_decay=d`` (0 = off) keeps an fp32 exponential moving average of every parameter in a fourth arena
  (``self.ema``), updated by the fused optimizer launch itself from the masters it holds in registers (one more read and
  write of the arena, no extra pass; a one-thread tick advances the device count ``ema_t`` that the warm-up
  d_n = min(d, (1 + n) / (10 + n)) reads, so a captured step needs nothing new).  ``ema_weights()`` swaps the
  average into the model for evaluation and checkpointing and swaps the raw weights back (README "EMA weights").

CU budget of the gradient all-reduce (``comm_ctas``, default 8 = parallel.reducer.DEFAULT_COMM_CTAS): the owned RCCL
communicator is created with ncclConfig_t.minCTAs = maxCTAs = comm_ctas, so its kernels occupy exactly that many of
the 256 CUs while they run beside the backward's two compute streams (RCCL's default picks its channel count for
bandwidth alone).  Sizing at the headline shape (batch 8 per GPU, 768x1024, 8 GPUs): a ring all-reduce moves
2 (W-1)/W x 82.9 MB = 145 MB per GPU per step; one channel (one workgroup) sustains a few tens of GB/s over an xGMI
link, so 8 channels move it in well under 1 ms, while the ~9 ms backward hands the buckets over progressively (the
backend's 40.5 MiB bucket is ready after ~3 ms).  Every bucket but the last therefore finishes under compute at 8
CUs = 3 % of the chip; only the last bucket (<= 1 MiB: conv1_x / conv2_x, split off by plan_buckets) is exposed after
the backward, ~2 MB of ring traffic = a few tens of microseconds.  More CTAs would shorten that tail by microseconds
while taking more CUs from the compute streams for the whole overlap; fewer would let the 40 MiB bucket run past the
backward on slow links.  ``bench.py --comm-ctas`` / ``train.py --comm-ctas`` set it (0 = RCCL's default), and bench.py
reports it in its N > 1 JSON line.
"""
from __future__ import annotations

import collections
import contextlib
import sys
from typing import Optional

import torch
import torch.distributed as dist

from ..models.cannet import CANNet
from ..ops import _ext
from ..ops.executor import CANNetExecutor
from ..utils.flat import FlatArena
from ..utils.profiling import trace_range
from .trainer import check_ema_decay

ACT_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


class SplitCapture:
    """One input shape's captured step as one graph per stream, launched in dependency order:

    * compute graph A: forward, fused head, the backward's data-gradient chain, and an event-record node at every
      fork (executor._on_side) and bucket mark (native reducer);
    * side graph: the weight gradients, each behind an event-wait node on its fork's event, then a record of its end
      (executor._join);
    * comm graph (native RCCL reducer): each bucket's all-reduce behind event-wait nodes on its producers' marks, then
      a record of its end (BucketReducer.finish);
    * compute graph B: event waits on the side graph's and the comm graph's ends, then the loss all-reduce, fused
      SGD + weight packs (and the fp16 overflow check / loss-scale update).

    Each graph is one chain, so each replays on its own launch stream the way the eager step's streams run.  One
    graph holding every branch (the torch.cuda.graph capture of the fork / join pattern) is replayed by the runtime's
    parallel-branch scheduler, which overlapped the branches less than the eager streams (round 4: 497.5 vs
    517.5 img/s, profiles/r4/graph_queues.txt) unless the HIP debug variable DEBUG_HIP_FORCE_GRAPH_QUEUES serialised
    it.  Launch order A, side, comm, B matters: a wait node takes the event's latest record at the time the graph
    holding it is launched, so every graph is launched after the graphs whose records it waits on; every fork owns
    its event and every bucket event is recorded once per step, so no later record of the same event can satisfy an
    earlier wait."""

    def __init__(self, C, side_stream: int, comm_stream: Optional[int] = None):
        self.C = C
        self.side = side_stream
        self.comm = comm_stream
        self.fork_events = []
        self.end_event = C.event_create()
        self.side_graph = self.side_exec = 0
        self.comm_graph = self.comm_exec = 0
        self.a = None
        self.b = None

    def fork(self, dst: int, src: int):
        ev = self.C.event_create()
        self.fork_events.append(ev)
        self.C.record_external(ev, src)
        self.C.wait_external(dst, ev)

    def side_end(self, side: int):
        self.C.record_external(self.end_event, side)

    def replay(self):
        self.a.replay()
        self.C.graph_launch(self.side_exec, self.side)
        if self.comm_exec:
            self.C.graph_launch(self.comm_exec, self.comm)
        self.b.replay()

    def summary(self, which: str = "side") -> dict:
        """Node counts of the side (or comm) graph and whether it is one chain (tests)."""
        return dict(self.C.graph_summary(self.side_graph if which == "side" else self.comm_graph))

    def __del__(self):
        C = getattr(self, "C", None)
        if C is None or sys.is_finalizing():          # at interpreter exit the process releases everything
            return
        try:
            torch.cuda.synchronize()
            # the compute graphs hold the record / wait nodes of the events: release them first, events last
            for g in (self.a, self.b):
                if g is not None:
                    g.reset()
            self.a = self.b = None
            C.graph_destroy(self.side_graph, self.side_exec)
            C.graph_destroy(self.comm_graph, self.comm_exec)
            self.side_graph = self.side_exec = self.comm_graph = self.comm_exec = 0
            for ev in self.fork_events + [self.end_event]:
                C.event_destroy(ev)
            self.fork_events = []
        except Exception:
            pass


OPTIMIZERS = ("sgd", "adam", "adamw")


class NativeStepper:
    def __init__(self, device, dtype="bf16", world=1, lr=1e-7, momentum=0.95, batch=8, height=768, width=1024,
                 graph=True, model: Optional[CANNet] = None, reducer=None, bucket_mb: float = 25.0,
                 reducer_transport: Optional[str] = None, init_scale="auto", scale_interval: int = 2000,
                 graph_max_shapes: int = 8, comm_ctas: Optional[int] = None, graph_bind_inputs: bool = False,
                 optimizer: str = "sgd", weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 accum_steps: int = 1, clip_grad_norm: float = 0.0, ema_decay: float = 0.0, ema_warmup: bool = True):
        check_ema_decay(ema_decay)
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")
        if int(accum_steps) != accum_steps or accum_steps < 1:
            raise ValueError(f"accum_steps must be an integer >= 1, got {accum_steps!r}")
        if not clip_grad_norm >= 0:
            raise ValueError(f"clip_grad_norm must be >= 0 (0 = off, inf = measure only), got {clip_grad_norm!r}")
        if dtype not in ACT_DTYPES:
            raise ValueError(f"the native step computes in bf16 or fp16 (fp32 master weights), got {dtype!r}; "
                             "use --impl torch for fp32")
        self.C = _ext.require()
        self.dtype = dtype
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.model = (model or CANNet(backend="hip")).to(self.device)
        self.model.exec_backend = "hip"
        self.world = world
        self.momentum = momentum
        self.optimizer = optimizer
        self.weight_decay = float(weight_decay)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.params = list(self.model.parameters())
        self.ex = CANNetExecutor(self.model, dtype=ACT_DTYPES[dtype])
        self.model._executor = self.ex
        # fp32 master/grad arenas laid out in gradient-ready order (contiguous buckets)
        self.arena = FlatArena(self.params, self.device, order=self.ex.grad_ready_order())
        self.mom = torch.zeros_like(self.arena.data)  # momentum buffer (zero init == torch's first-step clone)
        # Adam / AdamW: self.mom is the first moment; the second moment and the device count of applied steps (the
        # kernel's bias correction reads it, so a captured step advances it on replay) exist only for them
        self.mom2 = torch.zeros_like(self.arena.data) if optimizer != "sgd" else None
        self.opt_t = torch.zeros(1, dtype=torch.int32, device=self.device) if optimizer != "sgd" else None
        self.grads = self.arena.grad_views()
        # EMA of the parameters (0 = off: no arena, and the step launches the kernel without EMA): filled from the
        # masters at the end of the constructor, once the weights are final (after the rank-0 broadcast)
        self.ema_decay = float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema = torch.zeros_like(self.arena.data) if self.ema_decay > 0 else None
        self.ema_t = torch.zeros(1, dtype=torch.int32, device=self.device) if self.ema is not None else None
        self._ema_in = False                         # inside ema_weights(): the arena holds the average
        self.ex.opt_prepare(self.arena.data, self.arena.grad, self.mom, self.mom2, self.ema)   # (device descriptor: before any capture)
        # [non-finite loss (any rank after the all-reduce), loss, non-finite gradient (fp16), sticky non-finite]
        self.flags = torch.zeros(4, dtype=torch.float32, device=self.device)
        # gradient accumulation: a window of accum_steps micro-steps is ONE optimizer step on the sum of their
        # gradients (the loss is a sum-reduced MSE, so that is the batch's gradient: no 1/k, and lr is NOT rescaled
        # by accum_steps).  _micro = micro-steps run in the open window; _acc = the window's loss so far (device)
        self.accum_steps = int(accum_steps)
        self._micro = 0
        self._acc = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._warm = set()                           # input shapes an eager step or a capture warm-up has run
        # global-norm clipping (0 = off): the norm pass over the accumulated, all-reduced gradient right before the
        # optimizer, which reads the clip coefficient from the device (gn[1])
        self.clip_grad_norm = float(clip_grad_norm)
        self.gn = None
        if self.clip_grad_norm > 0:
            self.gn = self.ex.norm_prepare(self.arena.grad, [self.arena.offsets[i] for i in self.arena.order])
        self._lr_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.lr = lr * world                       # train.py:25 linear scaling
        # fp16: device-side dynamic loss scale {S, 1/S, clean steps, 0}
        self.scaler = None
        self.scale_interval = scale_interval
        # init_scale="auto" (fp16, default): the first step() first backs the scale off from 2^16 on its own batch
        # until the gradients are finite (probe backward passes, no update), then starts 4x below that.  With a fixed
        # 2^16 the sum-reduced MSE's large early gradients cost GradScaler-style skipped updates exactly during the
        # first-steps transient: 4 of the first 5 updates skipped while fp32 moved (loss 2532 vs 12453 at step 2);
        # auto: scale 1024, none skipped, the loss tracks fp32 (12512 vs 12453) (profiles/r5/grad_fidelity.md)
        self._auto_scale = dtype == "fp16" and init_scale == "auto"
        if self._auto_scale:
            init_scale = 65536.0
        if dtype == "fp16":
            init_scale = float(init_scale)
            self.scaler = torch.tensor([init_scale, 1.0 / init_scale, 0.0, 0.0], dtype=torch.float32,
                                       device=self.device)
        self.bucket_mb = bucket_mb
        self.comm_timing = False
        self._comm_events = []
        self._bucket_reports = []
        self.reducer = reducer
        if self.reducer is None and (world > 1 or reducer_transport is not None):
            from ..parallel.reducer import BucketedReducer, DEFAULT_COMM_CTAS
            self.reducer = BucketedReducer(self.arena, self.ex.grad_ready_order(), bucket_mb=bucket_mb,
                                           transport=reducer_transport or "auto",
                                           comm_priority=0 if graph else 1,
                                           comm_ctas=DEFAULT_COMM_CTAS if comm_ctas is None else comm_ctas)
        self.reducer_transport = None if self.reducer is None else self.reducer.transport
        if world > 1:
            self._broadcast_params()
        if self.ema is not None:
            self.ema.copy_(self.arena.data)
        if graph not in (True, False, "auto"):
            raise ValueError(f"graph must be True, False or 'auto', got {graph!r}")
        self.use_graph = graph
        # hipGraph-captured steps, one per input shape (LRU, at most graph_max_shapes): a dataset of a few image
        # sizes replays a graph per size instead of re-capturing whenever the size changes
        self.graph_max_shapes = graph_max_shapes
        # graph_bind_inputs: a captured step reads the caller's own input tensors (one graph per input buffer, keyed by
        # address; the caller keeps them alive and refills them in place, e.g. a double-buffered loader) instead of a
        # private copy refreshed by a device copy before every replay (two copy kernels per step: 0.4 % of a batch-1
        # step, profiles/r6/README.md)
        self.graph_bind_inputs = graph_bind_inputs
        self._graphs = collections.OrderedDict()     # shape key -> (graph, static img, static gt, static loss)
        self._seen = collections.Counter()
        self.graph = None
        self.static_img = None
        self.static_gt = None
        self._loss = None
        self.steps = 0
        self.graph_captures = 0

    # ------------------------------------------------------------ helpers
    def _broadcast_params(self):
        """Init-time consistency (train.py:98-114 + DDP ctor broadcast) in ONE collective."""
        if self.reducer is not None:
            self.reducer.broadcast_arena(0)
        else:
            dist.broadcast(self.arena.data, src=0)
        self.ex.refresh_packs(force=True)

    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, v: float):
        """Host value + the device scalar the SGD kernel reads (a captured step sees updates)."""
        self._lr = float(v)
        self._lr_dev.fill_(self._lr)

    # A micro-step's phase within its accumulation window is (opening, closing); accum_steps = 1: always WHOLE.
    #   opening: head and backward overwrite the gradient arena (beta 0), later micro-steps add to it (beta 1);
    #   closing: the reducer runs and the full tail follows (loss tick, loss / flag all-reduce, norm pass or overflow
    #   check, optimizer, loss-scale update); a non-closing micro-step leaves the reducer idle and its tail is the
    #   loss tick alone (the side stream is still joined before the next forward).
    WHOLE = (True, True)

    def _phase(self):
        return (self._micro == 0, self._micro + 1 >= self.accum_steps)

    def _step_body(self, img, gt, update: bool = True, phase=WHOLE):
        self._step_fwd_bwd(img, gt, phase)
        return self._step_tail(update, phase)

    def _step_fwd_bwd(self, img, gt, phase=WHOLE):
        """Forward, fused head + loss, backward (gradients into the arena, buckets handed to the reducer)."""
        ex = self.ex
        beta = 0.0 if phase[0] else 1.0
        with trace_range("cannet/forward"):
            b6, sv = ex.forward_features(img, save=True)
            ex.workspace(*ex.input_hw(img))
            sc = self.scaler
            # fused head: loss -> flags[1], its non-finite flag -> flags[0] (same kernel, no extra launch)
            loss, et, d_b6 = ex.head_train(b6, gt, self.grads, lscale=sc[0:1] if sc is not None else None,
                                           flags=self.flags, beta=beta)
        red = self.reducer if phase[1] else None
        timing = self.comm_timing and self.device.type == "cuda"
        if red is not None:
            red.set_timing(timing)
            red.begin()
            red.mark_ready([ex.head_w_index, ex.head_b_index])
        with trace_range("cannet/backward"):
            ex.backward_features(sv, d_b6, self.grads, on_grad_ready=(red.mark_ready if red is not None else None),
                                 dscale=sc[1:2] if sc is not None else None, beta=beta)
        del sv

    def _step_tail(self, update: bool = True, phase=WHOLE, fold: bool = True):
        """All-reduce join, fp16 overflow check, fused SGD + weight packs, loss-scale update.  Accumulation: the loss
        tick first; a non-closing micro-step ends there (returns None)."""
        ex = self.ex
        st = _ext.stream_ptr(self.device)
        sc = self.scaler
        red = self.reducer
        if self.accum_steps > 1 and update:
            self.C.accum_tick(self.flags.data_ptr(), self._acc.data_ptr(), (1 if phase[0] else 2) if fold else 0,
                              int(phase[1]), st)
        if not phase[1]:
            return None
        timing = self.comm_timing and self.device.type == "cuda"
        if timing:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        if red is not None:
            with trace_range("cannet/allreduce"):
                red.finish()
                red.allreduce_scalars(self.flags[0:2])
        if timing:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self._comm_events.append((e0, e1))
            if red is not None:
                self._bucket_reports.append(red.timings())
        clip = self.gn is not None
        if clip:
            # the norm of the accumulated, all-reduced gradient (every rank: the same value); a non-finite element
            # sets flags[2], so in fp16 this one read of the arena is also the overflow check
            self.flags[2:3].zero_()
            ex.grad_norm(1.0 / self.world, self.clip_grad_norm, self.flags)
        elif sc is not None:
            # after the all-reduce every rank holds the same gradients -> the same verdict
            self.flags[2:3].zero_()
            self.C.grad_nonfinite(self.arena.grad.data_ptr(), self.arena.numel, self.flags.data_ptr() + 8, st)
        if not update:
            return self.flags[1:2]
        with trace_range("cannet/sgd"):
            # the optimizer over the arena and the 16-bit weight packs in ONE launch (executor.opt_step)
            ex.opt_step(self.arena.data, self.arena.grad, self.mom, self._lr, 1.0 / self.world,
                        optimizer=self.optimizer, momentum=self.momentum, weight_decay=self.weight_decay,
                        betas=self.betas, eps=self.eps, mom2=self.mom2, step=self.opt_t, flags=self.flags,
                        lr_dev=self._lr_dev, gmul=self.gn[1:2] if clip else None, ema=self.ema, ema_t=self.ema_t,
                        ema_decay=self.ema_decay, ema_warmup=self.ema_warmup)
            if sc is not None:
                self.C.scale_update(self.flags.data_ptr() + 8, sc.data_ptr(), int(self.scale_interval), 2.0, 0.5,
                                    float(2 ** 24), st)
        return self.flags[1:2]

    def exposed_comm_ms(self, reset: bool = True) -> Optional[float]:
        """Mean device time between 'every gradient written' and 'all-reduce joined back' over the steps run
        with ``comm_timing`` (the part of the gradient all-reduce NOT hidden behind the backward)."""
        if not self._comm_events:
            return None
        torch.cuda.synchronize(self.device)
        v = sum(a.elapsed_time(b) for a, b in self._comm_events) / len(self._comm_events)
        if reset:
            self._comm_events = []
        return v

    def comm_report(self, reset: bool = True) -> Optional[dict]:
        """Per-bucket all-reduce timing of the last step run with ``comm_timing`` (BucketedReducer.timings: when
        each bucket's gradients were ready, when its all-reduce started / ended, relative to the start of the
        backward, and how long the all-reduce ran past the backward)."""
        t = [x for x in self._bucket_reports if x is not None]
        if reset:
            self._bucket_reports = []
        return t[-1] if t else None

    def calibrate_loss_scale(self, img, gt, headroom: float = 4.0, max_backoffs: int = 40) -> float:
        """fp16: back the loss scale off (x0.5) from its current value until this batch's gradients are finite
        (probe steps without update; host-synchronous, call outside a captured region), then divide by
        ``headroom``.  Returns the new scale."""
        if self.scaler is None:
            return 1.0
        for _ in range(max_backoffs):
            self._eager_body(img, gt, update=False)
            if float(self.flags[2]) == 0:
                break
            self.scaler[0:2].mul_(torch.tensor([0.5, 2.0], device=self.device))
        s = max(1.0, float(self.scaler[0]) / headroom)
        self.scaler.copy_(torch.tensor([s, 1.0 / s, 0.0, 0.0], device=self.device))
        self.flags.zero_()
        return s

    # ------------------------------------------------------------ public
    # per-GPU input pixels up to which graph="auto" replays captured steps: below it the eager step is host-bound
    # (~100 kernel launches + the executor's Python per step: batch 1 at 768x1024 ran 270 img/s eager,
    # profiles/r4/ragged); above it the eager two-stream step overlaps better than the replay (profiles/r4)
    AUTO_GRAPH_PIXELS = 2 * 768 * 1024

    def _wants_graph(self, img) -> bool:
        if self.use_graph is True:
            return True
        if self.use_graph is False:
            return False
        n, h, w = self.ex.input_hw(img)
        return n * h * w <= self.AUTO_GRAPH_PIXELS

    def step(self, img, gt):
        """One micro-step.  Returns the loss (summed over ranks; with accum_steps > 1: over the window's micro-batches
        too) as a device scalar on the call that closes a window, None on the others.  ``skipped_last()``, the sticky
        non-finite flag, Adam's step count and the fp16 loss scale all advance per window."""
        if self._ema_in:
            raise RuntimeError("step() inside ema_weights(): the model holds the averaged weights")
        if img.device != self.device:
            img = img.to(self.device, non_blocking=True)
        if gt.device != self.device:
            gt = gt.to(self.device, non_blocking=True)
        if self._auto_scale:
            self._auto_scale = False
            self.calibrate_loss_scale(img, gt)
        shape_key = key = (tuple(img.shape), img.dtype, tuple(gt.shape))
        if self.graph_bind_inputs:
            key += (img.data_ptr(), gt.data_ptr())
        phase = self._phase()
        if self.accum_steps > 1:
            key += (phase,)                  # a window's phases differ in beta and in the tail: one graph each
        use = self._wants_graph(img)
        if use and self.use_graph == "auto" and key not in self._graphs:
            # auto: capture a shape on its SECOND occurrence (a one-off size of a mixed-size set runs eager)
            self._seen[key] += 1
            use = self._seen[key] >= 2
        ent = self._graphs.get(key) if use else None
        if use and ent is None and not phase[0] and shape_key not in self._warm:
            # a shape first met inside an open window: _capture's warm-up (a real forward / backward into the
            # gradient arena) would clobber the window, so this occurrence runs eagerly as the real micro-step --
            # the same kernels on the same shapes, which is all the warm-up is for -- and the next one captures
            use = False
        if not use:
            out = self._eager_body(img, gt, phase=phase)
            self._warm.add(shape_key)
            return self._advance(out, phase)
        if ent is None:
            ent = self._capture(img, gt, key, phase=phase, warm=shape_key not in self._warm or phase[0])
            self._warm.add(shape_key)
        else:
            self._graphs.move_to_end(key)
        self.graph, self.static_img, self.static_gt, self._static_loss = ent
        if self.static_img.data_ptr() != img.data_ptr():
            self.static_img.copy_(img, non_blocking=True)
        if self.static_gt.data_ptr() != gt.data_ptr():
            self.static_gt.copy_(gt, non_blocking=True)
        self.graph.replay()
        return self._advance(self._static_loss, phase)

    def _advance(self, out, phase):
        self.steps += 1
        self._micro = 0 if phase[1] else self._micro + 1
        if phase[1]:
            self._loss = out
        return out

    def flush(self):
        """Close an open accumulation window now (the end of an epoch: no sample is dropped, nothing leaks into the
        next epoch, a checkpoint never sees an open window): the reducer over the accumulated arena, then the full
        tail, eagerly.  Returns the window's loss, or None when no window is open."""
        if self._micro == 0:
            return None
        red = self.reducer
        if red is not None:
            red.set_timing(False)
            red.begin()
            red.mark_ready(list(self.arena.order))
        out = self._step_tail(True, phase=(False, True), fold=False)
        self._micro = 0
        self._loss = out
        return out

    # ------------------------------------------------------------ EMA
    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model holds the EMA weights: one swap launch exchanges the master arena with the EMA
        arena and re-packs (the parameters are views of the arena, so ``model(img)``, ``state_dict()`` and
        ``save_checkpoint`` see the average; no address changes, captured graphs stay valid); the exit swaps back, bit
        for bit.  Raises inside an open accumulation window (call ``flush()`` first) and when EMA is off."""
        if self.ema is None:
            raise RuntimeError("ema_weights(): EMA is off (ema_decay = 0)")
        if self._micro != 0:
            raise RuntimeError("ema_weights(): an accumulation window is open; call flush() first")
        if self._ema_in:
            raise RuntimeError("ema_weights() does not nest")
        self.ex.swap_weights(self.arena.data, self.ema)
        self._ema_in = True
        try:
            yield self.model
        finally:
            self.ex.swap_weights(self.arena.data, self.ema)
            self._ema_in = False

    def ema_state(self) -> Optional[dict]:
        """{"ema": {parameter name: averaged tensor (a clone)}, "steps": updates applied}, keyed like ``state_dict``;
        None when EMA is off."""
        if self.ema is None:
            return None
        src = self.arena.data if self._ema_in else self.ema
        out = {}
        for (name, _), (off, n), p in zip(self.model.named_parameters(), self.arena.offsets, self.params):
            out[name] = src[off:off + n].view_as(p).clone()
        return {"ema": out, "steps": int(self.ema_t.item())}

    def load_ema_state(self, ema: Optional[dict], steps: int = 0) -> bool:
        """Restore the average from a name-keyed dict (either stepper family's ``ema_state()["ema"]``); None: restart
        it from the current weights at n = 0.  Returns whether a saved average was loaded."""
        if self.ema is None:
            return False
        if not ema:
            self.ema.copy_(self.arena.data)
            self.ema_t.zero_()
            return False
        for (name, _), (off, n) in zip(self.model.named_parameters(), self.arena.offsets):
            self.ema[off:off + n].copy_(ema[name].reshape(-1).to(self.device))
        self.ema_t.fill_(int(steps))
        return True

    def grad_norm(self) -> Optional[float]:
        """Global 2-norm of the last window's accumulated, averaged gradient, before clipping (None: clipping off).
        Synchronises the host, as ``grad_norms`` and ``clip_coef``: meant for the logging cadence."""
        return None if self.gn is None else float(self.gn[0].item())

    def clip_coef(self) -> Optional[float]:
        """The coefficient the last window's gradient was multiplied by (0: skipped on a non-finite gradient)."""
        return None if self.gn is None else float(self.gn[1].item())

    def grad_norms(self) -> Optional[dict]:
        """Parameter name -> 2-norm of its gradient in the last window."""
        if self.gn is None:
            return None
        names = [n for n, _ in self.model.named_parameters()]
        v = self.gn[2:].tolist()
        return {names[i]: v[j] for j, i in enumerate(self.arena.order)}

    def _ws_ptr(self):
        ws = self.ex.ws
        return None if ws is None else ws.buf.data_ptr()

    def _eager_body(self, img, gt, update: bool = True, phase=WHOLE):
        """An eager step; if it grew the shared weight-gradient workspace (a larger shape), every captured graph
        points at the released buffer and is dropped."""
        before = self._ws_ptr()
        # (the step on a high-priority stream measured -1 % at batch 1, profiles/r5/ab_hp_step.jsonl: removed)
        out = self._step_body(img, gt, update=update, phase=phase)
        if self._graphs and self._ws_ptr() != before:
            self._graphs.clear()
        return out

    def _capture(self, img, gt, key=None, phase=WHOLE, warm: bool = True):
        """warm = False: the shape has run before (its opening phase's warm-up or an eager micro-step), and this
        phase's capture must not run a real backward into the open window's gradient arena."""
        key = key if key is not None else (tuple(img.shape), img.dtype, tuple(gt.shape))
        while len(self._graphs) >= max(1, self.graph_max_shapes):
            self._graphs.popitem(last=False)             # LRU: its graph and private memory pool are released
        static_img = img if self.graph_bind_inputs else img.clone()
        static_gt = gt if self.graph_bind_inputs else gt.clone()
        # warm up on a side stream (allocations, workspace sizing, kernel attrs); a grown workspace drops the
        # graphs captured before (_eager_body)
        if warm:
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):
                self._eager_body(static_img, static_gt, update=False)
            torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        side = self.ex._side_stream()
        nat = getattr(self.reducer, "_native", None) if self.reducer is not None else None
        if side is not None and (self.reducer is None or nat is not None):
            # (a non-closing micro-step leaves the reducer idle: no comm graph)
            g, loss = self._capture_split(static_img, static_gt, side.cuda_stream, nat if phase[1] else None, phase)
        else:
            # torch-transport reducer (its collectives are torch.distributed works) or no side stream: one graph
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._shared_pool()):
                loss = self._step_body(static_img, static_gt, phase=phase)
        torch.cuda.synchronize(self.device)
        ent = (g, static_img, static_gt, loss)
        self._graphs[key] = ent
        self.graph_captures += 1
        return ent

    def _shared_pool(self):
        """ONE memory pool for every captured step of this stepper (all shapes, both compute graphs): a replay runs to
        completion on its streams before the next replay's first graph starts (graph B waits for the side and comm
        graphs' ends, the next A follows B on the compute stream), so a later capture may reuse the temporaries of an
        earlier one, and a cache of many shapes (a mixed-size dataset, graph_max_shapes) holds about one step's
        activations instead of one per shape.  Persistent state (arena, packs, workspace, inputs) lives outside it."""
        if getattr(self, "_graph_pool", None) is None:
            self._graph_pool = torch.cuda.graph_pool_handle()
        return self._graph_pool

    def _capture_split(self, static_img, static_gt, side: int, nat=None, phase=WHOLE):
        """Capture the step as compute graph A + side graph (+ comm graph) + compute graph B (SplitCapture).
        nat: the native RCCL BucketReducer, whose comm stream is captured as its own graph spanning A and B (its
        bucket all-reduces are issued during A, its end is recorded by finish() during B)."""
        C, ex = self.C, self.ex
        comm = nat.comm_stream if nat is not None else None
        sc = SplitCapture(C, side, comm)
        a, b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        ex.split = sc
        comm_open = False
        if nat is not None:
            nat.set_split(True)
        try:
            with torch.cuda.graph(a, pool=self._shared_pool(), capture_error_mode="relaxed"):
                C.capture_begin(side)
                if comm is not None:
                    C.capture_begin(comm)
                    comm_open = True
                try:
                    self._step_fwd_bwd(static_img, static_gt, phase)
                finally:
                    sc.side_graph = C.capture_end(side)
            # (not torch.cuda.graph: its __enter__ synchronises the device, which a stream still capturing -- the
            # comm graph spans A and B -- forbids)
            if getattr(self, "_cap_stream", None) is None:
                self._cap_stream = _ext.own_stream(self.device)
            with torch.cuda.stream(self._cap_stream):
                b.capture_begin(pool=self._shared_pool(), capture_error_mode="relaxed")
                try:
                    C.wait_external(_ext.stream_ptr(self.device), sc.end_event)
                    loss = self._step_tail(True, phase)
                finally:
                    b.capture_end()
        finally:
            if comm_open:
                sc.comm_graph = C.capture_end(comm)
            ex.split = None
            if nat is not None:
                nat.set_split(False)
        sc.side_exec = C.graph_instantiate(sc.side_graph)
        if comm is not None:
            sc.comm_exec = C.graph_instantiate(sc.comm_graph)
        sc.a, sc.b = a, b
        return sc, loss

    def resume_state(self) -> dict:
        """Device state a resumed run needs besides weights and momentum (checkpoint.save_train_state)."""
        st = {"lr": self._lr, "steps": self.steps, "optimizer": self.optimizer, "momentum": float(self.momentum),
              "weight_decay": self.weight_decay, "beta1": self.betas[0], "beta2": self.betas[1], "eps": self.eps}
        if self.opt_t is not None:
            st["opt_steps"] = int(self.opt_t.item())
        if self.scaler is not None:
            st["scaler"] = self.scaler
        if self.ema is not None:
            st.update(ema_steps=int(self.ema_t.item()), ema_decay=self.ema_decay, ema_warmup=self.ema_warmup)
        return st

    def load_resume_state(self, st: Optional[dict]):
        if not st:
            return
        saved = st.get("optimizer", "sgd")             # (a state from before the optimizer choice: SGD)
        if saved != self.optimizer:
            raise ValueError(f"the saved state is a {saved!r} run, this stepper runs {self.optimizer!r}: their "
                             "optimizer states are not interchangeable")
        if self.opt_t is not None:
            self.opt_t.fill_(int(st.get("opt_steps", 0)))
        self.lr = float(st.get("lr", self._lr))
        self.steps = int(st.get("steps", self.steps))
        if self.scaler is not None and st.get("scaler") is not None:
            self.scaler.copy_(st["scaler"].to(self.scaler.device))
        if self.ema is not None and st.get("ema_steps") is not None:
            self.ema_t.fill_(int(st["ema_steps"]))
        self.ex.refresh_packs(force=True)

    def last_loss(self) -> Optional[float]:
        return None if self._loss is None else float(self._loss.reshape(-1)[0])

    def nonfinite(self) -> bool:
        """A non-finite loss in ANY step since the last ``reset_nonfinite()`` (the reference's exit condition,
        utils/train_eval_utils.py:48-50; sticky on the device, so polling every k steps misses none).  An fp16
        gradient overflow is not one: that step is skipped and the loss scale backed off."""
        return bool(self.flags[3].item() != 0)

    def reset_nonfinite(self):
        self.flags[3:4].zero_()

    def loss_scale(self) -> float:
        return 1.0 if self.scaler is None else float(self.scaler[0].item())

    def skipped_last(self) -> bool:
        """True when the last step's update was skipped (non-finite loss or gradient)."""
        f = self.flags.tolist()
        return f[0] != 0 or f[2] != 0
