#!/usr/bin/env python
"""Distributed CANNet training (reference: train.py of zgzhengSEU/CAN-distributed-pytorch).

Launch exactly like the reference (one process per GPU, env rendezvous):
    python -m torch.distributed.run --nproc_per_node=8 --master-addr 127.0.0.1 train.py --data_root data/SHA/
    python train.py --synthetic 768x1024 --epochs 2          # single GPU, synthetic data
All reference flags are accepted with the same names and defaults (train.py:174-197);
booleans parse properly (--wandb false works; reference Q2), --data_root is honoured
(ShanghaiTech layout {train,test}_data/{images,ground_truth}; reference Q3).

Per epoch: train (native fused step: HIP kernels + RCCL bucketed reducer +
fused SGD), distributed MAE evaluation (sum over ranks / padded test-set size,
reference train.py:157), best-MAE checkpoint ``checkpoints/epoch_{e}.pth``
(plain CANNet state_dict, loadable by test.py and by the reference's test.py),
a resumable ``checkpoints/last_state.pth``, JSONL metrics.
"""
from __future__ import annotations

import argparse
import contextlib
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from can_distributed_pytorch_amd.models import CANNet  # noqa: E402
from can_distributed_pytorch_amd.parallel.distributed import init_distributed_mode, barrier, cleanup  # noqa: E402
from can_distributed_pytorch_amd.utils.checkpoint import (save_checkpoint, load_checkpoint,  # noqa: E402
                                                          save_train_state, load_train_state)
from can_distributed_pytorch_amd.utils.metrics import JsonlLogger, wandb_init, wandb_log  # noqa: E402


def str2bool(v):
    if isinstance(v, bool):
        return v
    if str(v).lower() in ("1", "true", "yes", "y", "t"):
        return True
    if str(v).lower() in ("0", "false", "no", "n", "f"):
        return False
    raise argparse.ArgumentTypeError(f"boolean expected, got {v!r}")


def graph_mode(v):
    if str(v).lower() == "auto":
        return "auto"
    return str2bool(v)


def accum_count(v):
    n = int(v)
    if n < 1:
        raise argparse.ArgumentTypeError(f"--accum-steps must be >= 1, got {v!r}")
    return n


def clip_norm(v):
    x = float(v)
    if not x >= 0:
        raise argparse.ArgumentTypeError(f"--clip-grad-norm must be >= 0 (0 = off, inf = measure only), got {v!r}")
    return x


def ema_decay(v):
    x = float(v)
    if not 0.0 <= x < 1.0:
        raise argparse.ArgumentTypeError(f"--ema-decay must be in [0, 1) (0 = off), got {v!r}")
    return x


def crop_size(v):
    try:
        h, w = (int(x) for x in str(v).lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--crop-size expects HxW, got {v!r}")
    if h <= 0 or w <= 0 or h % 8 or w % 8:
        raise argparse.ArgumentTypeError(f"--crop-size must be positive multiples of 8 (the density downsample), got {v!r}")
    return h, w


def crop_scale(v):
    try:
        lo, hi = (float(x) for x in str(v).split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--crop-scale expects LO,HI, got {v!r}")
    if not (0.0 < lo <= hi) or lo < 0.25 or hi > 4.0:
        raise argparse.ArgumentTypeError(f"--crop-scale must satisfy 0.25 <= LO <= HI <= 4, got {v!r}")
    return lo, hi


def photo_jitter(v):
    try:
        b, c, g = (float(x) for x in str(v).split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--photo-jitter expects B,C,G, got {v!r}")
    if not (0.0 <= b <= 0.5 and 0.0 <= c <= 1.0 and 1.0 <= g <= 2.0):
        raise argparse.ArgumentTypeError(f"--photo-jitter must satisfy 0 <= B <= 0.5, 0 <= C <= 1, 1 <= G <= 2, got {v!r}")
    return b, c, g


def gray_prob(v):
    p = float(v)
    if not 0.0 <= p <= 1.0:
        raise argparse.ArgumentTypeError(f"--gray-prob must be in [0, 1], got {v!r}")
    return p


def crop_count(v):
    n = int(v)
    if n < 1:
        raise argparse.ArgumentTypeError(f"--crops-per-image must be >= 1, got {v!r}")
    return n


def game_level(v):
    n = int(v)
    if not 0 <= n <= 3:
        raise argparse.ArgumentTypeError(f"--eval-game must be a level 0..3, got {v!r}")
    return n


class _Parser(argparse.ArgumentParser):
    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if ns.crop_size is not None and ns.synthetic:
            self.error("--crop-size crops decoded dataset images; it cannot be combined with --synthetic")
        if ns.roi_masks and ns.synthetic:
            self.error("--roi-masks reads the dataset's ground_truth/NAME.roi.npy masks; it cannot be combined with "
                       "--synthetic")
        if ns.crop_scale is not None and ns.crop_size is None:
            self.error("--crop-scale rescales the windows of --crop-size; give --crop-size as well")
        if ns.gt_from_heads and ns.crop_size is None:
            self.error("--gt-from-heads renders the ground truth of the crops of --crop-size; give --crop-size as well")
        for flag, value in (("--photo-jitter", ns.photo_jitter), ("--gray-prob", ns.gray_prob)):
            if value is not None and ns.synthetic:
                self.error(f"{flag} jitters the crops of decoded dataset images; it cannot be combined with --synthetic")
            if value is not None and ns.crop_size is None:
                self.error(f"{flag} jitters the colours of the crops of --crop-size; give --crop-size as well")
        return ns


def build_parser():
    p = _Parser(description="CANNet training on MI355X")
    # ---- reference flags (same names / defaults)
    p.add_argument("--epochs", type=int, default=500)
    p.add_argument("--batch-size", type=int, default=1)
    p.add_argument("--lr", type=float, default=1e-7)
    p.add_argument("--optimizer", choices=["sgd", "adam", "adamw"], default="sgd",
                   help="sgd: torch.optim.SGD semantics (the reference); adam / adamw: torch.optim.Adam / AdamW "
                        "(coupled / decoupled --weight-decay).  Every optimizer runs as one fused native kernel with "
                        "--impl hip and as the torch.optim one with --impl torch; --lr is multiplied by the world "
                        "size for every optimizer (the reference's rule)")
    p.add_argument("--momentum", type=float, default=0.95, help="SGD momentum")
    p.add_argument("--weight-decay", type=float, default=0.0)
    p.add_argument("--accum-steps", type=accum_count, default=1,
                   help="gradient accumulation: one optimizer step per window of this many batches, on the SUM of "
                        "their gradients (the loss is sum-reduced, so a window of k batch-1 steps of any image sizes "
                        "is one batch-k step of the reference's loss; --lr is NOT rescaled by k).  A window still "
                        "open at the end of an epoch is closed there")
    p.add_argument("--clip-grad-norm", type=clip_norm, default=0.0,
                   help="clip the global 2-norm of the (accumulated, averaged) gradient to this value ahead of the "
                        "optimizer, torch.nn.utils.clip_grad_norm_'s rule; 0 (default) = off, inf = measure the norm "
                        "only (logged as grad_norm)")
    p.add_argument("--ema-decay", type=ema_decay, default=0.0,
                   help="keep an exponential moving average of the weights with this decay and evaluate / checkpoint "
                        "it instead of the raw weights (epoch_N.pth then holds the average, last_state.pth the raw "
                        "weights plus the average); usual range 0.999-0.9999; 0 (default) = off")
    p.add_argument("--ema-warmup", type=str2bool, default=True,
                   help="with --ema-decay: use min(decay, (1 + n) / (10 + n)) at the n-th update, so the average "
                        "follows the weights early on")
    p.add_argument("--beta1", type=float, default=0.9, help="Adam / AdamW first-moment decay")
    p.add_argument("--beta2", type=float, default=0.999, help="Adam / AdamW second-moment decay")
    p.add_argument("--eps", type=float, default=1e-8, help="Adam / AdamW epsilon")
    p.add_argument("--lrf", type=float, default=0.1, help="final lr factor for --lr-schedule cosine (unused otherwise, as in the reference)")
    p.add_argument("--syncBN", type=str2bool, default=True,
                   help="convert BatchNorm to SyncBatchNorm when world > 1 (the reference model has no BN: a no-op "
                        "unless --batch-norm)")
    p.add_argument("--wandb", type=str2bool, default=True, help="log to wandb if it is installed")
    p.add_argument("--show", type=str2bool, default=True, help="save GT/prediction overlay PNGs each epoch")
    p.add_argument("--data_root", type=str, default="./data/Shanghai_part_A/")
    p.add_argument("--init_checkpoint", type=str, default="./checkpoints/epoch_26.pth")
    p.add_argument("--device", default="cuda")
    p.add_argument("--world-size", default=4, type=int)
    p.add_argument("--dist-url", default="env://")
    # ---- new flags
    p.add_argument("--impl", choices=["hip", "torch"], default="hip", help="hip: native kernels; torch: stock PyTorch (reference stack)")
    p.add_argument("--dtype", choices=["bf16", "fp32", "fp16"], default="bf16")
    p.add_argument("--synthetic", type=str, default="", help="HxW: train/eval on synthetic crowds of this size")
    p.add_argument("--synthetic-n", type=int, default=64, help="synthetic train-set size (test set = n/4)")
    p.add_argument("--graph", type=graph_mode, default=False,
                   help="capture the step, one graph per stream per input shape (LRU cache, --graph-cache): true = "
                        "always; auto = for small per-GPU inputs (<= 2 x 768x1024 pixels), on the second occurrence of "
                        "a shape; false (default) = eager.  The captured step replays at eager speed "
                        "(profiles/r6/ab_graph_split_bound.jsonl): the step is GPU-bound at batch 1 too "
                        "(profiles/r6/train_b1/)")
    p.add_argument("--graph-cache", type=int, default=1024,
                   help="captured steps kept (one per input shape, LRU; they share one memory pool, so a mixed-size "
                        "dataset's shapes all fit)")
    p.add_argument("--bucket-mb", type=float, default=25.0)
    p.add_argument("--comm-ctas", type=int, default=None,
                   help="CU budget of the RCCL gradient all-reduce (default 8, engine/native.py; 0 = RCCL default)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--num-workers", type=int, default=8, help="JPEG-decoding DataLoader workers per rank")
    p.add_argument("--lr-schedule", choices=["none", "cosine"], default="none")
    p.add_argument("--checkpoint-dir", default="checkpoints")
    p.add_argument("--resume", type=str, default="", help="resume from a last_state.pth written by this script")
    p.add_argument("--log-jsonl", type=str, default="checkpoints/metrics.jsonl")
    p.add_argument("--vgg16", type=str, default="", help="local torchvision VGG-16 state_dict for the frontend (reference downloads it)")
    p.add_argument("--eval-every", type=int, default=1)
    p.add_argument("--check-sync-every", type=int, default=1, help="epochs between cross-rank weight fingerprint checks (0: off)")
    p.add_argument("--batch-norm", type=str2bool, default=False,
                   help="make_layers(batch_norm=True) variant (reference C04 branch; stock autograd path only)")
    p.add_argument("--gpu-preprocess", type=str2bool, default=True,
                   help="decode on CPU workers, resize/flip/normalise on the GPU (hip impl, real data)")
    p.add_argument("--crop-size", type=crop_size, default=None, metavar="HxW",
                   help="train on random HxW crops (multiples of 8) instead of whole images: any integer offset, a "
                        "p=0.5 flip per crop, an image smaller than the crop is zero-padded at the bottom / right "
                        "(the padding takes part in the loss, unless --roi-masks weights it out).  Every training batch then has one shape, so "
                        "--batch-size > 1 works on a mixed-size dataset; evaluation stays on whole images at batch 1.  "
                        "Default: off")
    p.add_argument("--crops-per-image", type=crop_count, default=1,
                   help="with --crop-size: crops cut from every decoded image (one decode, one copy); a step sees "
                        "batch-size x this many samples and the loss is sum-reduced, so choose --lr as for that many "
                        "images (as with --accum-steps)")
    p.add_argument("--crop-scale", type=crop_scale, default=None, metavar="LO,HI",
                   help="with --crop-size: every crop draws a scale s log-uniformly on [LO, HI] (0.25 <= LO <= HI <= 4, "
                        "e.g. 0.75,1.33) and resamples a window of the crop size / s to the crop (s > 1 magnifies), "
                        "bilinearly, the density rescaled by the area ratio.  The window always fits: an image smaller "
                        "than the crop is upsampled to fill it, not padded.  Default: off")
    p.add_argument("--gt-from-heads", action="store_true",
                   help="with --crop-size (with or without --crop-scale): render every crop's ground truth from the "
                        "image's head records (ground_truth/IMG_k.heads.npy, written by data_preparation/"
                        "k_nearest_gaussian_kernel.py <root> --heads) as exact area sums of the density map, on the GPU "
                        "with --gpu-preprocess, instead of point-sampling the map: a cell holds its window's density "
                        "mass at any scale.  Default: off")
    p.add_argument("--photo-jitter", type=photo_jitter, default=None, metavar="B,C,G",
                   help="with --crop-size: every crop draws a brightness shift uniform on [-B, B] (0 <= B <= 0.5, of the "
                        "0..1 range), a contrast factor log-uniform on [1/(1+C), 1+C] about mid-gray (0 <= C <= 1) and a "
                        "gamma log-uniform on [1/G, G] (1 <= G <= 2), e.g. 0.2,0.3,1.5; they act on the source pixels as "
                        "one 256-entry tone table per crop, inside the crop launch with --gpu-preprocess.  Training "
                        "crops only.  Default: off")
    p.add_argument("--gray-prob", type=gray_prob, default=None, metavar="P",
                   help="with --crop-size: every crop is turned gray (luma 0.299 R + 0.587 G + 0.114 B in all three "
                        "channels, after the tone table of --photo-jitter) with this probability.  Default: off")
    p.add_argument("--roi-masks", action="store_true",
                   help="the dataset has a region-of-interest mask per image (ground_truth/NAME.roi.npy: uint8 [H, W], "
                        "255 inside, 0 outside): the loss is weighted per cell by the mask's exact area mean (0 in the "
                        "padding of a crop too), counts are taken inside the mask, and the epoch records gain rmse.  "
                        "The weights are rendered on the GPU with --gpu-preprocess.  Default: off")
    p.add_argument("--eval-game", type=game_level, default=None, metavar="L",
                   help="evaluate with the grid average mean absolute error GAME(1..L) as well (0 <= L <= 3; GAME(0) "
                        "is the MAE), logged as game1..gameL next to mae and rmse.  Default: off")
    p.add_argument("--log-every", type=int, default=20,
                   help="steps between the training records of --log-jsonl (each reads the loss back: a host sync)")
    return p


def make_loaders(args, world, rank, raw=False, device=None, dtype=None):
    """Train / test loaders.  raw=True: decoded uint8 samples packed per batch in the workers (PackedCollate),
    one H2D copy + one preprocessing launch per batch on the GPU.  Synthetic data on a GPU run is rendered on
    the GPU (SyntheticGPULoader), sharded by the same DistributedSampler."""
    from torch.utils.data import DataLoader, DistributedSampler, BatchSampler
    from can_distributed_pytorch_amd.data import CrowdDataset, SyntheticCrowdDataset
    from can_distributed_pytorch_amd.data.dataset import EpochTaggedSampler
    from can_distributed_pytorch_amd.ops.preprocess import PackedCollate
    collate = PackedCollate() if raw else None
    crop = args.crop_size
    train_collate, eval_batch = collate, args.batch_size
    photo = args.photo_jitter is not None or args.gray_prob is not None
    if crop is not None:
        # every training sample is a crop of one size; test images stay whole and of mixed size: batch 1
        from can_distributed_pytorch_amd.data.dataset import crop_collate
        train_collate = PackedCollate(crop=crop, crop_scale=args.crop_scale is not None,
                                      gt_from_heads=args.gt_from_heads, photo=photo) if raw else crop_collate
        eval_batch = 1
    if args.synthetic:
        h, w = (int(v) for v in args.synthetic.lower().split("x"))
        train_ds = SyntheticCrowdDataset(args.synthetic_n, h, w, seed=args.seed)
        test_ds = SyntheticCrowdDataset(max(1, args.synthetic_n // 4), h, w, seed=args.seed + 1)
    else:
        r = args.data_root
        train_ds = CrowdDataset(os.path.join(r, "train_data", "images"), os.path.join(r, "train_data", "ground_truth"),
                                gt_downsample=8, phase="train", seed=args.seed, raw=raw, crop=crop,
                                crops_per_image=args.crops_per_image if crop is not None else 1,
                                crop_scale=args.crop_scale, gt_from_heads=args.gt_from_heads,
                                **(dict(roi=True) if args.roi_masks else {}),
                                **(dict(photo_jitter=args.photo_jitter or (0.0, 0.0, 1.0),
                                        gray_prob=args.gray_prob or 0.0) if photo else {}))
        test_ds = CrowdDataset(os.path.join(r, "test_data", "images"), os.path.join(r, "test_data", "ground_truth"),
                               gt_downsample=8, phase="test", raw=raw, **(dict(roi=True) if args.roi_masks else {}))
    train_sampler = DistributedSampler(train_ds, num_replicas=world, rank=rank, shuffle=True, seed=args.seed)
    test_sampler = DistributedSampler(test_ds, num_replicas=world, rank=rank, shuffle=True, seed=args.seed)
    # indices carry the epoch into (persistent) workers: the flip is a function of (seed, epoch, index)
    bs = BatchSampler(EpochTaggedSampler(train_sampler), args.batch_size, drop_last=False)
    if args.synthetic and device is not None and device.type == "cuda" and args.impl == "hip" and \
            args.dtype != "fp32" and h % 16 == 0 and w % 16 == 0:
        from can_distributed_pytorch_amd.data.synthetic import SyntheticGPULoader
        train_loader = SyntheticGPULoader(bs, h, w, args.seed, device, dtype=dtype)
        test_loader = SyntheticGPULoader(BatchSampler(test_sampler, args.batch_size, drop_last=False), h, w,
                                         args.seed + 1, device, dtype=dtype)
        return train_loader, test_loader, train_sampler, test_sampler
    pin = torch.cuda.is_available()
    train_loader = DataLoader(train_ds, batch_sampler=bs, num_workers=args.num_workers, pin_memory=pin,
                              persistent_workers=args.num_workers > 0, collate_fn=train_collate,
                              prefetch_factor=4 if args.num_workers > 0 else None)
    test_loader = DataLoader(test_ds, sampler=test_sampler, batch_size=eval_batch, num_workers=args.num_workers,
                             pin_memory=pin, shuffle=False, collate_fn=collate)
    return train_loader, test_loader, train_sampler, test_sampler


def main(args):
    init_distributed_mode(args)
    rank, world = args.rank, args.world_size
    use_gpu = str(args.device).startswith("cuda") and torch.cuda.is_available()
    device = torch.device("cuda", args.gpu) if use_gpu else torch.device("cpu")
    if args.impl == "hip" and not use_gpu:
        print("[no GPU: falling back to --impl torch on CPU]")
        args.impl = "torch"
    if args.batch_norm and args.impl == "hip":
        print("[--batch-norm: the fused native step has no BN layers; using --impl torch]")
        args.impl = "torch"
    base_lr = args.lr
    torch.manual_seed(args.seed)
    os.makedirs(args.checkpoint_dir, exist_ok=True)
    log = JsonlLogger(args.log_jsonl, enabled=(rank == 0))
    use_wandb = rank == 0 and wandb_init(args.wandb, project="CANNet-MI355X", name="CANNet", config=vars(args))
    if rank == 0:
        print(f"[train start {time.strftime('%Y.%m.%d %H:%M:%S')}] world {world} impl {args.impl} {args}")

    # the NHWC4 16-bit input layout the GPU preprocessing writes is the native bf16/fp16 step's
    raw = bool(args.gpu_preprocess and args.impl == "hip" and args.dtype != "fp32" and not args.synthetic)
    act = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    train_loader, test_loader, train_sampler, test_sampler = make_loaders(args, world, rank, raw=raw, device=device,
                                                                          dtype=act)
    prep = None
    if raw:
        from can_distributed_pytorch_amd.ops.preprocess import AheadPrep, preprocess_packed
        copy_stream = torch.cuda.Stream(device) if torch.device(device).type == "cuda" else None
        roi_kw = dict(roi=True) if args.roi_masks else {}    # the packs carry the masks as alpha: gt [n, 2, h, w]
        prep = lambda b: preprocess_packed(b, device, dtype=act, copy_stream=copy_stream, **roi_kw)  # noqa: E731
        train_prep = AheadPrep(device, dtype=act, **roi_kw)  # training: the next batch one step ahead

    model = CANNet(vgg16_path=args.vgg16 or None, backend="hip" if args.impl == "hip" else "torch",
                   batch_norm=args.batch_norm)
    if args.syncBN and world > 1 and args.batch_norm:
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)      # train.py:116-118
    if os.path.exists(args.init_checkpoint):
        res = load_checkpoint(model, args.init_checkpoint, strict=False)
        if rank == 0:
            print(f"[load {args.init_checkpoint}: missing {len(res.missing_keys)} unexpected {len(res.unexpected_keys)}]")
    # init-weight consistency (train.py:98-114 + DDP broadcast): one collective in the stepper
    from can_distributed_pytorch_amd.engine.trainer import build_trainer
    graph = args.graph
    # the fused native stepper (flat arena, RCCL reducer, device lr) runs --impl hip in bf16 / fp16; every other
    # combination (--impl torch, and --impl hip --dtype fp32 = Fp32Stepper) is a TorchStepper with a torch optimizer
    native = args.impl == "hip" and args.dtype != "fp32"
    opt = dict(optimizer=args.optimizer, momentum=args.momentum, weight_decay=args.weight_decay,
               betas=(args.beta1, args.beta2), eps=args.eps, accum_steps=args.accum_steps,
               clip_grad_norm=args.clip_grad_norm, ema_decay=args.ema_decay, ema_warmup=args.ema_warmup)
    ema_on = args.ema_decay > 0
    if native:
        stepper = build_trainer(impl="hip", dtype=args.dtype, device=device, world=world, lr=base_lr, graph=graph,
                                model=model, bucket_mb=args.bucket_mb, comm_ctas=args.comm_ctas,
                                graph_max_shapes=args.graph_cache, **opt)
        net = stepper.model
        momentum, momentum2 = stepper.mom, stepper.mom2
    else:
        # --impl torch: stock ATen / MIOpen; --impl hip --dtype fp32: split-bf16 convolutions on the native
        # MFMA kernels (engine/trainer.Fp32Stepper), the rest of the step as the torch one
        stepper = build_trainer(impl=args.impl, dtype=args.dtype if use_gpu else "fp32", device=device, world=world,
                                lr=base_lr, model=model, bucket_mb=args.bucket_mb, **opt)
        if world > 1:
            for p in stepper.model.parameters():
                dist.broadcast(p.data, src=0)
            stepper.ema_start()                      # the average starts from the weights as broadcast
        net = stepper.net
        momentum = momentum2 = None

    start_epoch, min_mae, min_epoch = 0, float("inf"), 0
    if args.resume and os.path.exists(args.resume):
        rs = load_train_state(args.resume, stepper.model, momentum,
                              optimizer=None if native else stepper.opt, momentum2=momentum2,
                              optimizer_name=args.optimizer)
        start_epoch, min_mae, min_epoch = rs["epoch"] + 1, rs["min_mae"], rs["min_epoch"]
        if native:
            stepper.load_resume_state(rs["stepper"])
        if ema_on:
            if not stepper.load_ema_state(rs["ema"], rs["ema_steps"]) and rank == 0:
                print(f"[resume: {args.resume} has no EMA; the average starts from the loaded weights at n = 0]")
        elif rs["ema"] is not None and rank == 0:
            print(f"[resume: {args.resume} holds an EMA of the weights; ignored (--ema-decay 0)]")

    from can_distributed_pytorch_amd.engine.train_eval import train_one_epoch_native, evaluate, train_one_epoch
    import math
    for epoch in range(start_epoch, args.epochs):
        train_sampler.set_epoch(epoch)
        if args.lr_schedule == "cosine":
            f = ((1 + math.cos(epoch * math.pi / args.epochs)) / 2) * (1 - args.lrf) + args.lrf
            if native:
                stepper.lr = base_lr * world * f
            else:
                for g in stepper.opt.param_groups:
                    g["lr"] = base_lr * world * f
        t0 = time.perf_counter()
        if native:
            mean_loss = train_one_epoch_native(stepper, train_loader, device, epoch, log=log,
                                               log_every=max(1, args.log_every), prep=train_prep if raw else prep)
        else:
            mean_loss = train_one_epoch(net, stepper.opt, train_loader, device, epoch,
                                        accum_steps=args.accum_steps, clip_grad_norm=args.clip_grad_norm,
                                        **(dict(on_step=stepper.ema_update) if ema_on else {}))
        t_train = time.perf_counter() - t0
        # EMA on: evaluation, the overlay PNGs and the best-MAE checkpoint see the averaged weights (every rank swaps)
        averaged = stepper.ema_weights if ema_on else contextlib.nullcontext
        metrics_on = args.roi_masks or args.eval_game is not None
        extra = {}
        with averaged():
            evaluating = (epoch + 1) % args.eval_every == 0 or epoch == args.epochs - 1
            if evaluating and metrics_on:
                # masked counts, RMSE and GAME (engine/metrics.py): sums over the test set, one collective; the best
                # checkpoint is chosen by the masked MAE, GAME_0's mean
                from can_distributed_pytorch_amd.engine.metrics import evaluate_metrics
                ms = evaluate_metrics(net, test_loader, device, prep=prep)
                mae_sum = ms["game"][0]
                extra = dict(rmse=math.sqrt(ms["se"] / test_sampler.total_size),
                             **{f"game{l}": ms["game"][l] / test_sampler.total_size
                                for l in range(1, (args.eval_game or 0) + 1)})
            elif evaluating:
                mae_sum = evaluate(net, test_loader, device, epoch, show_images=args.show and rank == 0,
                                   use_wandb=use_wandb, out_dir=os.path.join(args.checkpoint_dir, "temp"), prep=prep)
            else:
                mae_sum = float("nan")
            mean_mae = mae_sum / test_sampler.total_size      # padded size, reference parity (Q6)
            if rank == 0 and mean_mae < min_mae:
                min_mae, min_epoch = mean_mae, epoch
                save_checkpoint(stepper.model, os.path.join(args.checkpoint_dir, f"epoch_{epoch}.pth"))
        if args.check_sync_every and (epoch + 1) % args.check_sync_every == 0 and world > 1:
            from can_distributed_pytorch_amd.parallel.consistency import check_replicas_consistent, check_comm_health
            if native:
                check_comm_health(stepper.reducer)
                check_replicas_consistent(stepper.arena.data)
                if ema_on:
                    check_replicas_consistent(stepper.ema)
            else:
                check_replicas_consistent(torch.cat([p.detach().reshape(-1) for p in stepper.model.parameters()]))
                if ema_on:
                    check_replicas_consistent(torch.cat([e.reshape(-1) for e in stepper.ema_state()["ema"].values()]))
        if rank == 0:
            es = stepper.ema_state() if ema_on else None
            save_train_state(os.path.join(args.checkpoint_dir, "last_state.pth"), stepper.model, momentum, epoch,
                             min_mae, optimizer=None if native else stepper.opt, min_epoch=min_epoch,
                             stepper_state=stepper.resume_state() if native else None, momentum2=momentum2,
                             optimizer_name=args.optimizer,
                             **(dict(ema=es["ema"], ema_steps=es["steps"], ema_decay=args.ema_decay) if es else {}))
            lr_now = stepper.lr if native else stepper.opt.param_groups[0]["lr"]
            per_item = args.crops_per_image if args.crop_size is not None else 1
            ips = len(train_loader) * args.batch_size * per_item * world / max(t_train, 1e-9)
            print(f"[epoch {epoch}] loss: {mean_loss:.4f} mae: {mean_mae:.3f}, min_mae: {min_mae:.3f}, "
                  f"min_epoch: {min_epoch}, train img/s {ips:.1f}")
            st = getattr(stepper, "last_epoch_stats", None) or {}
            log.log(kind="epoch", epoch=epoch, loss=mean_loss, mae=mean_mae, min_mae=min_mae, lr=lr_now,
                    train_imgs_per_s=ips, train_s=t_train, train_mpix_per_s=st.get("mpix_per_s"),
                    train_loop_imgs_per_s=st.get("imgs_per_s"), batch_size=args.batch_size, world=world,
                    **(dict(crop_size=list(args.crop_size), crops_per_image=args.crops_per_image,
                            eval_batch_size=test_loader.batch_size) if args.crop_size is not None else {}),
                    **(dict(crop_scale=list(args.crop_scale)) if args.crop_scale is not None else {}),
                    **(dict(gt_from_heads=True) if args.gt_from_heads else {}),
                    **(dict(photo_jitter=list(args.photo_jitter)) if args.photo_jitter is not None else {}),
                    **(dict(gray_prob=args.gray_prob) if args.gray_prob is not None else {}),
                    **(dict(ema_decay=args.ema_decay) if ema_on else {}),
                    **(dict(roi_masks=True) if args.roi_masks else {}), **extra)
            if use_wandb:
                wandb_log(loss=mean_loss, mae=mean_mae, lr=lr_now)
        barrier()
    cleanup()


if __name__ == "__main__":
    main(build_parser().parse_args())
