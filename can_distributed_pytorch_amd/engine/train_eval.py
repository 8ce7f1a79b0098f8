"""Epoch loops: training and distributed evaluation.

Parity: utils/train_eval_utils.py of the reference —
  * ``train_one_epoch(model, optimizer, train_loader, device, epoch)`` (:13-58):
    MSELoss(sum), loss reduced (averaged) over ranks, running-mean loss,
    non-finite guard -> exit(1), optimizer.step; returns the mean loss;
  * ``evaluate(model, test_loader, device, epoch, show_images, use_wandb)``
    (:61-138): mae += |sum(et) - sum(gt)| per batch, optional overlay PNGs of
    one random batch, SUM-reduced over ranks; returns the MAE sum.

Native fast path: ``train_one_epoch_native(stepper, ...)`` drives the fused
NativeStepper (HIP executor + RCCL reducer + fused SGD): no host sync per
step — the loss is read back only every ``log_every`` steps and the
non-finite flag (device-side, all-reduced with the loss, and latched by the
SGD kernel so a NaN on a step that is not read is never lost) is checked at
the same cadence and at the end of the epoch.
"""
from __future__ import annotations

import contextlib
import itertools
import random
import sys
import time
from typing import Optional

import torch

from ..parallel.distributed import is_main_process, reduce_value, get_world_size
from .metrics import weighted_sq_loss


def _progress(it, enabled):
    if not enabled:
        return it
    try:
        from tqdm import tqdm
        return tqdm(it, file=sys.stdout)
    except Exception:  # pragma: no cover
        return it


def train_one_epoch(model, optimizer, train_loader, device, epoch, log=None, accum_steps: int = 1,
                    clip_grad_norm: float = 0.0, on_step=None):
    """Generic autograd path (any model/optimizer, DDP or our hook reducer).

    accum_steps > 1: one optimizer step per window of accum_steps batches on the sum of their gradients (the loss is
    sum-reduced: no 1/k, lr not rescaled) -- zero_grad at a window's start, DDP ``no_sync()`` on its non-closing
    batches, and a window still open at the end of the epoch is closed there (for DDP the loader's last batch always
    runs synchronised, so that flush has the all-reduced gradient).  clip_grad_norm > 0:
    torch.nn.utils.clip_grad_norm_ ahead of every optimizer step.  on_step: called after every optimizer step (the
    EMA update of the stepper that owns the optimizer)."""
    model.train()
    criterion = weighted_sq_loss                  # MSELoss(sum); a 2-channel gt carries a loss weight
    mean_loss = torch.zeros(1, device=device)
    loader = _progress(train_loader, is_main_process())
    params = [p for p in model.parameters() if p.requires_grad]
    try:
        last = len(train_loader) - 1
    except TypeError:
        last = -1
    micro = 0

    def apply():
        if clip_grad_norm > 0:
            torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], clip_grad_norm)
        optimizer.step()
        if on_step is not None:
            on_step()

    for step, (img, gt) in enumerate(loader):
        if micro == 0:
            optimizer.zero_grad()
        closing = micro + 1 >= accum_steps or step == last
        img, gt = img.to(device, non_blocking=True), gt.to(device, non_blocking=True)
        with (model.no_sync() if not closing and hasattr(model, "no_sync") else contextlib.nullcontext()):
            et = model(img)
            loss = criterion(et, gt)
            loss.backward()
        micro = 0 if closing else micro + 1
        loss = reduce_value(loss.detach(), average=True)
        mean_loss = (mean_loss * step + loss) / (step + 1)
        if is_main_process() and hasattr(loader, "desc"):
            loader.desc = f"[epoch {epoch}] mean loss {round(mean_loss.item(), 3)}"
        if not torch.isfinite(loss):
            print("WARNING: non-finite loss, ending training ", loss)
            sys.exit(1)
        if closing:
            apply()
    if micro:
        apply()                                   # (a loader without a length: the open window's flush)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    return mean_loss.item()


def train_one_epoch_native(stepper, train_loader, device, epoch, log=None, log_every: int = 20, prep=None):
    """Fused native step per batch (see engine/native.py).  ``prep`` maps a raw
    loader batch to (img, gt) on the device (GPU preprocessing)."""
    stepper.model.train()
    stepper.reset_nonfinite()          # the device flag is sticky: any non-finite step of this epoch latches it
    loader = _progress(train_loader, is_main_process())
    total = torch.zeros(1, device=device)
    n = 0
    t0 = time.perf_counter()
    imgs = 0
    pix = 0
    ahead = prep is not None and hasattr(prep, "issue")      # ops/preprocess.py AheadPrep: one batch ahead
    it = iter(loader)
    first = next(it, None) if ahead else None                # (an empty loader: nothing to issue)
    pending = prep.issue(first) if first is not None else None
    clip = getattr(stepper, "clip_grad_norm", 0.0) > 0
    last_loss = None                                         # the latest closed window's loss (for the records)

    def add(loss):
        # a window's loss arrives on the call that closes it (None on the others); the running mean stays "sum of
        # losses / number of micro-batches", the reference's meaning at accum_steps = 1
        if loss is not None:
            total.add_(loss.reshape(1) / max(1, get_world_size()))
    for step in itertools.count():
        if ahead:
            if pending is None:
                break
            img, gt = prep.ready(pending)
            loss = stepper.step(img, gt)      # SUM of the per-rank losses (averaged below)
            nxt = next(it, None)              # the next batch's copy + preprocessing run under this step
            pending = prep.issue(nxt) if nxt is not None else None
        else:
            batch = next(it, None)
            if batch is None:
                break
            img, gt = prep(batch) if prep is not None else batch
            loss = stepper.step(img, gt)      # SUM of the per-rank losses (averaged below)
        add(loss)
        if loss is not None:
            last_loss = loss
        n += 1
        imgs += img.shape[0] * get_world_size()
        # NHWC4 (GPU-preprocessed) or NCHW input: per-pixel throughput for variable-size images
        hw = img.shape[1] * img.shape[2] if (img.dim() == 4 and img.shape[-1] == 4) else img.shape[-2] * img.shape[-1]
        pix += img.shape[0] * hw * get_world_size()
        if (step + 1) % log_every == 0:
            if stepper.nonfinite():
                print("WARNING: non-finite loss, ending training")
                sys.exit(1)
            if is_main_process():
                ml = (total / n).item()
                if hasattr(loader, "desc"):
                    loader.desc = f"[epoch {epoch}] mean loss {round(ml, 3)}"
                if log is not None:
                    dt = time.perf_counter() - t0
                    rec = dict(kind="train", epoch=epoch, step=step + 1, mean_loss=ml, imgs_per_s=imgs / max(dt, 1e-9),
                               input_shape=list(img.shape),
                               loss=None if last_loss is None else float(last_loss) / max(1, get_world_size()))
                    if clip:
                        rec.update(grad_norm=stepper.grad_norm(), clip_coef=stepper.clip_coef())
                    log.log(**rec)
    if hasattr(stepper, "flush"):
        add(stepper.flush())                      # an open accumulation window ends with the epoch
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    stepper.last_epoch_stats = {"imgs": imgs, "mpix": pix / 1e6, "seconds": dt,
                                "imgs_per_s": imgs / max(dt, 1e-9), "mpix_per_s": pix / 1e6 / max(dt, 1e-9)}
    if stepper.nonfinite():
        print("WARNING: non-finite loss, ending training")
        sys.exit(1)
    return (total / max(n, 1)).item()


@torch.no_grad()
def evaluate(model, test_loader, device, epoch, show_images=False, use_wandb=False, out_dir="checkpoints/temp",
             prep=None):
    model.eval()
    mae = torch.zeros(1, device=device)
    loader = _progress(test_loader, is_main_process())
    index = random.randint(0, max(0, len(test_loader) - 1))
    for step, batch in enumerate(loader):
        img, gt = prep(batch) if prep is not None else batch
        img, gt = img.to(device, non_blocking=True), gt.to(device, non_blocking=True)
        et = model(img)
        mae += torch.abs(et.sum() - gt.sum())
        if is_main_process():
            if hasattr(loader, "desc"):
                loader.desc = f"[epoch {epoch}]"
            if show_images and step == index:
                from ..utils.vis import save_overlays
                im0 = img[0]
                if im0.dim() == 3 and im0.shape[-1] == 4:          # NHWC4 bf16 -> CHW float
                    im0 = im0[..., :3].float().permute(2, 0, 1)
                paths = save_overlays(im0, gt[0], et[0], epoch, out_dir)
                if use_wandb:
                    from ..utils.metrics import wandb_log_images
                    wandb_log_images(paths, epoch)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    mae_sum = reduce_value(mae, average=False)
    return mae_sum.item()


@torch.no_grad()
def evaluate_per_image(model, loader, device):
    """Single-process per-image MAE / RMSE (test.py:cal_mae semantics)."""
    model.eval()
    ae, se, n = 0.0, 0.0, 0
    for img, gt in loader:
        img, gt = img.to(device), gt.to(device)
        et = model(img)
        d = (et.flatten(1).sum(1) - gt.flatten(1).sum(1)).double()
        ae += d.abs().sum().item()
        se += (d * d).sum().item()
        n += img.shape[0]
    return ae / max(n, 1), (se / max(n, 1)) ** 0.5
