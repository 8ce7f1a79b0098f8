#!/usr/bin/env python
"""Headline benchmark: CANNet training throughput (imgs/sec, whole node).

Config (BASELINE.json): CANNet, ShanghaiTech-shape synthetic 768x1024 (HxW)
crowd images, per-GPU batch 8 (weak scaling: global batch = 8*N), bf16
compute with fp32 master weights, MSE(sum) loss, SGD momentum 0.95,
lr 1e-7*world (train.py:25,63 of the reference), data-parallel over RCCL.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``.
  * launched by torch.distributed.run (WORLD_SIZE set): one rank per GPU;
    WORLD_SIZE must equal --gpus (else exit 2 — never a silent 1-GPU number);
  * launched bare with --gpus N > 1: this process spawns the N ranks itself
    (``python -m torch.distributed.run --nproc-per-node N``) BEFORE touching
    the GPU and exits with their status; fewer than N visible GPUs -> exit 2.
W untimed steps, then exactly K timed steps bracketed by barrier +
synchronize; the max over ranks is reported; rank 0 prints ONE JSON line.

``--device cpu`` rehearses the same chain without a GPU (gloo, this framework's
flat-arena data-parallel engine on the plain-ATen model, tiny default shape):
``bench.py --device cpu --gpus 2`` goes launch_ranks -> torchrun -> rank main
-> max-reduced JSON exactly as the driver's N-GPU run does (tests/test_bench_contract.py).

Every timed step is a full training step: H2D-free synthetic batch already
resident (data="synthetic"), forward, loss, backward, gradient all-reduce,
optimizer step.  A plain run does nothing else: set up, W warm-up steps, the K
timed steps, the JSON line.  ``--full`` adds, after the timed region (not
timed): a few steps with hipEvents around the all-reduce join
(``exposed_allreduce_ms``, per-bucket ``allreduce_timeline``), the cross-rank
replica fingerprint check (``replicas_consistent``; diverged replicas exit
non-zero), the reducer's description and the peak HBM of the run.
``--impl torch`` measures the stock PyTorch-ROCm reference stack (MIOpen convs
+ torch DDP) on the same config for comparison.

``--dump-outputs DIR`` writes, after the timed steps, what the last timed step
handed its caller, as float32 ``DIR/<name>.npy`` (``sample_index`` float64;
rank 0's replica): train mode
``loss`` (the step's return value) and a fixed seeded sample of the updated
parameters (``params``) and of their gradients (``grads``), gathered in
``model.parameters()`` order at the element indices in ``sample_index``; infer
mode ``density`` (the estimated density maps).  Weights, batches and the sample
are seeded, so two builds run with the same arguments compare file for file.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BASELINE_IMGS_PER_SEC = 119.692  # stock PyTorch-ROCm bf16 stack on 1x MI355X (reference publishes none)
METRIC = "imgs/sec (whole node) + ShanghaiTech-A MAE, CANNet at 1/2/4/8 MI355X"


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch", type=int, default=None, help="per-GPU batch (default 8; cpu: 2)")
    p.add_argument("--height", type=int, default=None, help="default 768 (cpu: 64)")
    p.add_argument("--width", type=int, default=None, help="default 1024 (cpu: 64)")
    p.add_argument("--device", choices=["cuda", "cpu"], default="cuda",
                   help="cpu: gloo rehearsal of the multi-rank chain (--impl arena by default)")
    p.add_argument("--impl", choices=["hip", "torch", "arena"], default=None,
                   help="hip: native kernels + RCCL reducer (cuda default); torch: stock PyTorch + DDP; "
                        "arena: plain-ATen model + this framework's flat-arena bucketed reducer (cpu default)")
    p.add_argument("--dtype", choices=["bf16", "fp32", "fp16"], default="bf16")
    p.add_argument("--bucket-mb", type=float, default=25.0, help="gradient all-reduce bucket cap (MiB)")
    p.add_argument("--comm-ctas", type=int, default=None,
                   help="CU budget of the owned RCCL communicator (ncclConfig_t.minCTAs = maxCTAs; default 8, see "
                        "engine/native.py; 0 = RCCL's default channel count)")
    p.add_argument("--reducer", choices=["rccl", "torch"], default=os.environ.get("CANNET_REDUCER", "rccl"),
                   help="rccl: own C++ RCCL communicator + bucketed reducer; torch: torch.distributed (NCCL=RCCL)")
    p.add_argument("--graph", default="0", choices=["0", "1", "auto"],
                   help="hipGraph-capture the step (hip impl): 1 always, 0 never (default: the eager step is faster "
                        "at batch 8 and at batch 1, profiles/r4, profiles/r5), auto for per-GPU inputs <= 2 x 768x1024 "
                        "pixels (engine/native.py AUTO_GRAPH_PIXELS)")
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run the untimed diagnostics (all-reduce timing steps, replica "
                        "consistency check, reducer description, peak HBM) and report them in the JSON line")
    p.add_argument("--comm-steps", type=int, default=3,
                   help="--full: extra untimed steps with all-reduce timing events")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's outputs to DIR/<name>.npy (float32)")
    p.add_argument("--mode", choices=["train", "infer"], default="train",
                   help="train: the headline training step; infer: forward-only density estimation (serving)")
    # test-only: rank 1 perturbs one weight of its replica after the timed steps, so the replica check must fail
    # and the run must exit non-zero (tests/test_bench_contract.py); never set by the driver
    p.add_argument("--test-desync", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args(argv)
    a.graph = {"0": False, "1": True}.get(a.graph, a.graph)
    cpu = a.device == "cpu"
    if a.impl is None:
        a.impl = "arena" if cpu else os.environ.get("CANNET_BENCH_IMPL", "hip")
    if cpu and a.impl == "hip":
        p.error("--impl hip needs --device cuda")
    if cpu and a.dtype != "fp32":
        a.dtype = "fp32"                       # the CPU rehearsal computes in fp32
    a.batch = a.batch or (2 if cpu else 8)
    a.height = a.height or (64 if cpu else 768)
    a.width = a.width or (64 if cpu else 1024)
    return a


def visible_gpu_count() -> int:
    """GPUs this process may use, counted WITHOUT initialising HIP (torch.cuda.device_count() can fall back to
    hipGetDeviceCount, and a process that has touched the GPU must not start the rank processes).

    KFD topology nodes with SIMDs are the GPUs; one counts only if its render node /dev/dri/renderD<minor> is
    accessible (a container sees only the devices it was given), then ROCR_/HIP_/CUDA_VISIBLE_DEVICES narrow it."""
    base = "/sys/class/kfd/kfd/topology/nodes"
    n = 0
    try:
        nodes = os.listdir(base)
    except OSError:
        nodes = []
    n_nodes = 0
    for node in nodes:
        try:
            props = dict(line.split()[:2] for line in open(os.path.join(base, node, "properties")) if line.strip())
        except (OSError, ValueError):
            continue
        if int(props.get("simd_count", "0")) <= 0:
            continue                           # a CPU node
        n_nodes += 1
        minor = props.get("drm_render_minor")
        if minor is not None and not os.access(f"/dev/dri/renderD{minor}", os.R_OK | os.W_OK):
            continue
        n += 1
    if n_nodes == 0:
        # no readable KFD topology (a container without /sys/class/kfd): ask HIP in a short-lived child process,
        # so this launcher process itself still never initialises the GPU
        try:
            r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"],
                               capture_output=True, text=True, timeout=300)
            n = int(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 and r.stdout.strip() else 0
        except (OSError, ValueError, subprocess.TimeoutExpired):
            n = 0
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([x for x in v.split(",") if x.strip()]))
    return n


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(a) -> int:
    """--gpus N without a launcher: spawn N ranks with torch.distributed.run.  Nothing here touches the GPU (no torch
    import even): the GPUs are counted from the KFD topology (visible_gpu_count)."""
    if a.device == "cuda":
        n_vis = visible_gpu_count()
        if n_vis < a.gpus:
            print(f"bench.py: --gpus {a.gpus} requested but only {n_vis} GPU(s) visible; refusing to report a "
                  f"different node size", file=sys.stderr)
            return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


DUMP_SAMPLE = 1 << 21      # elements per sampled array: 8 MB of float32 each, far below the 64 MB a dump may take


def dump_outputs(path: str, arrays: dict) -> None:
    """``path/<name>.npy`` per array, float32 (float64 inputs stay float64)."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        if isinstance(t, torch.Tensor):
            t = t.detach().to("cpu", torch.float64 if t.dtype == torch.float64 else torch.float32).numpy()
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(t))


def train_outputs(trainer, loss) -> dict:
    """What the last step handed its caller: the returned loss, and the parameters it updated in place with their
    gradients -- every element when that fits DUMP_SAMPLE, else the elements at a fixed seeded sample of indices into
    the concatenation of ``model.parameters()`` (independent of the arena's layout)."""
    import numpy as np
    import torch
    params = list(trainer.model.parameters())
    total = sum(p.numel() for p in params)
    if total <= DUMP_SAMPLE:
        index = np.arange(total, dtype=np.int64)
    else:
        index = np.sort(np.random.default_rng(0).integers(0, total, DUMP_SAMPLE, dtype=np.int64))
    idx = torch.from_numpy(index).to(params[0].device)

    def sample(ts):
        return torch.cat([t.detach().reshape(-1).float() for t in ts])[idx]
    return {"loss": loss.detach().reshape(-1), "params": sample(params),
            "grads": sample([p.grad if p.grad is not None else torch.zeros_like(p) for p in params]),
            "sample_index": index.astype(np.float64)}


def infer(a, trainer, pool, sync_all, world, rank, local, dev, cpu) -> int:
    """Forward-only throughput (test.py's density estimation): eval mode, no autograd, the same kernels as the
    training forward (native: executor.forward_eval + the 1x1 head)."""
    import torch
    import torch.distributed as dist
    model = trainer.model
    model.eval()
    cast = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(a.dtype) if a.impl == "torch" else None
    imgs = [p[0] for p in pool]

    def fwd(x):
        with torch.no_grad():
            if cast is not None:
                with torch.autocast("cuda", dtype=cast):
                    return model(x.contiguous(memory_format=torch.channels_last))
            return model(x)
    for i in range(a.warmup):
        fwd(imgs[i % len(imgs)])
    sync_all()
    t0 = time.perf_counter()
    for i in range(a.steps):
        et = fwd(imgs[i % len(imgs)])
    sync_all()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, {"density": et})
    if rank == 0:
        print(json.dumps({
            "metric": "CANNet inference imgs/sec (forward only, density map)", "value": round(a.batch * world * a.steps / dt, 3),
            "unit": "imgs/sec", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(1000.0 * dt / a.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
            "config": {"model": "CANNet", "global_batch": a.batch * world, "per_gpu_batch": a.batch,
                       "image_hw": [a.height, a.width], "impl": a.impl, "mode": "infer"},
            "count_first_image": float(et[0].sum())}), flush=True)
    if world > 1:
        dist.barrier(**({} if cpu else {"device_ids": [local]}))
        dist.destroy_process_group()
    return 0


def diagnostics(a, trainer, pool, sync_all, world, rank, dev, cpu, graph_used) -> dict:
    """--full: the untimed diagnostics after the timed region (extra fields of the JSON line)."""
    import torch
    import torch.distributed as dist
    extra = {}
    red = getattr(trainer, "reducer", None)
    native = a.impl == "hip" and a.dtype != "fp32"       # hip + fp32 = split-bf16 convs under the torch step
    if native or a.impl == "arena":
        extra["reducer"] = None if red is None else red.transport
        if native:
            extra["rccl_world"] = (red.comm.world if (red is not None and red.comm is not None) else
                                   (1 if red is None else None))
            # the all-reduce's CU budget (ncclConfig_t.minCTAs = maxCTAs; 0 = RCCL's default; None: no owned comm)
            extra["comm_ctas"] = None if red is None else red.comm_ctas
        extra["buckets_mib"] = None if red is None else [round(b.numel * 4 / 2 ** 20, 3) for b in red.buckets]
        if a.comm_steps > 0 and not graph_used:
            trainer.comm_timing = True
            for i in range(a.comm_steps):
                trainer.step(*pool[i % len(pool)])
            trainer.comm_timing = False
            if native:
                ms_comm = trainer.exposed_comm_ms()
                extra["exposed_allreduce_ms"] = None if ms_comm is None else round(ms_comm, 4)
            # per-bucket all-reduce timeline of the last diagnostic step (ms after the backward started), max over
            # ranks of the exposed tail: shows whether the all-reduce kernels got CUs while the backward ran
            rep = trainer.comm_report()
            if rep is not None:
                ex_t = torch.tensor([rep["exposed_ms"]], dtype=torch.float64, device=dev)
                if world > 1:
                    dist.all_reduce(ex_t, op=dist.ReduceOp.MAX)
                rep["exposed_ms_max_over_ranks"] = round(float(ex_t), 4)
            extra["allreduce_timeline"] = rep
        sync_all()
        from can_distributed_pytorch_amd.parallel.consistency import check_replicas_consistent
        if a.test_desync and rank == 1:
            with torch.no_grad():
                trainer.arena.data[:1].add_(1.0)
        try:
            extra["replicas_consistent"] = bool(check_replicas_consistent(trainer.arena.data))
        except RuntimeError as e:
            extra["replicas_consistent"] = False
            print(f"bench.py: {e}", file=sys.stderr)
    if not cpu:
        peak = torch.tensor([torch.cuda.max_memory_allocated(dev), torch.cuda.max_memory_reserved(dev)],
                            device=dev, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(peak, op=dist.ReduceOp.MAX)
        extra["peak_hbm_gb"] = {"allocated": round(float(peak[0]) / 1e9, 3),
                                "reserved": round(float(peak[1]) / 1e9, 3)}
    return extra


def main(argv=None) -> int:
    a = parse(argv)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and a.gpus > 1:
        return launch_ranks(a)
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}: refusing to mislabel the run", file=sys.stderr)
        return 2

    # whether the timed step is a hipGraph replay (auto: the per-GPU input is small enough that the eager step is
    # host-bound, engine/native.py NativeStepper.AUTO_GRAPH_PIXELS)
    graph_used = a.impl == "hip" and a.dtype != "fp32" and a.device == "cuda" and (
        a.graph is True or (a.graph == "auto" and a.batch * a.height * a.width <= 2 * 768 * 1024))
    import torch
    import torch.distributed as dist
    cpu = a.device == "cpu"
    if cpu:
        dev = torch.device("cpu")
        if world > 1:
            dist.init_process_group("gloo")
    else:
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
        if world > 1:
            dist.init_process_group("nccl", device_id=dev)

    from can_distributed_pytorch_amd.engine.trainer import build_trainer
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch, expected_flops_per_image

    torch.manual_seed(0)
    transport = None if a.reducer == "rccl" else "torch"
    trainer = build_trainer(impl=a.impl, dtype=a.dtype, device=dev, world=world, lr=1e-7, batch=a.batch,
                            height=a.height, width=a.width, graph=a.graph, bucket_mb=a.bucket_mb,
                            reducer_transport=transport, comm_ctas=a.comm_ctas,
                            graph_bind_inputs=True)   # replays read the resident pool batches in place
    # a small pool of distinct synthetic batches, resident on the GPU
    pool = [make_synthetic_batch(a.batch, a.height, a.width, seed=1000 * rank + i, device=dev) for i in range(2)]

    def sync_all():
        if world > 1:
            dist.barrier(**({} if cpu else {"device_ids": [local]}))
        if not cpu:
            torch.cuda.synchronize()

    if a.mode == "infer":
        return infer(a, trainer, pool, sync_all, world, rank, local, dev, cpu)

    for i in range(a.warmup):
        trainer.step(*pool[i % len(pool)])
    sync_all()
    t0 = time.perf_counter()
    for i in range(a.steps):
        trainer.step(*pool[i % len(pool)])
    sync_all()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    loss = trainer.last_loss()

    # ---- what the last timed step handed back, then (--full) the untimed diagnostics
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, train_outputs(trainer, trainer._loss))
    extra = diagnostics(a, trainer, pool, sync_all, world, rank, dev, cpu, graph_used) if a.full else {}

    # self-policing for the driver's N-GPU run: a run whose replicas diverged, or whose own RCCL communicator does
    # not span every rank, is not a valid data-parallel measurement -> non-zero exit on every rank
    problems = []
    if world > 1 and extra.get("replicas_consistent") is False:
        problems.append("replicas diverged (cross-rank weight fingerprints differ)")
    if world > 1 and a.impl == "hip" and a.dtype != "fp32" and a.reducer == "rccl":
        # (checked in a plain run too: it reads one attribute of the communicator the timed steps used)
        comm = getattr(getattr(trainer, "reducer", None), "comm", None)
        if comm is None or comm.world != world:
            problems.append(f"RCCL communicator spans {None if comm is None else comm.world} rank(s), not {world}")
    bad = torch.tensor([float(len(problems))], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
    if float(bad) > 0 and not problems:
        problems.append("another rank reported an invalid run")
    if problems:
        extra["invalid"] = problems
        print(f"bench.py: INVALID data-parallel run: {'; '.join(problems)}", file=sys.stderr)

    ms = 1000.0 * dt / a.steps
    imgs = a.batch * world * a.steps / dt
    tflops = 3.0 * expected_flops_per_image(a.height, a.width) * imgs / 1e12
    if rank == 0:
        out = {
            "metric": METRIC,
            "value": round(imgs, 3),
            "unit": "imgs/sec",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(ms, 3),
            "higher_is_better": True,
            "scaling": "weak",
            # stock stack measured on 1 GPU; for N GPUs it is credited with perfect (N x) scaling
            "vs_baseline": (round(imgs / (BASELINE_IMGS_PER_SEC * world), 4) if BASELINE_IMGS_PER_SEC else None),
            "dtype": a.dtype,
            "data": f"synthetic (random-init weights, synthetic {a.height}x{a.width} crowd images + "
                    f"count-preserving 1/8 density maps)",
            "config": {"model": "CANNet", "global_batch": a.batch * world, "per_gpu_batch": a.batch,
                       "image_hw": [a.height, a.width], "seq_len": None,
                       "parallelism": f"dp{world}", "impl": a.impl, "device": a.device,
                       "graph": bool(graph_used), "bucket_mb": a.bucket_mb,
                       "optimizer": "SGD(m=0.95) fp32 master", "loss": "MSE(sum)"},
            "train_tflops_per_s": round(tflops, 2),
            "final_loss": loss,
        }
        out.update(extra)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier(**({} if cpu else {"device_ids": [local]}))
        dist.destroy_process_group()
    return 3 if problems else 0


if __name__ == "__main__":
    rc = main()
    # the stepper / executor / model reference each other: collect them now, so the RCCL communicator, graphs and
    # streams they own are released while the runtime is up, not during interpreter teardown
    gc.collect()
    sys.exit(rc)
