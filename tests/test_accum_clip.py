"""Gradient accumulation and global-norm clipping on the CPU side: the command line, the stock steppers (TorchStepper,
ArenaStepper), the paused reducer on two gloo ranks, the epoch loops and train.py end to end."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _model(seed=0):
    from can_distributed_pytorch_amd.models import CANNet
    torch.manual_seed(seed)
    return CANNet(backend="torch")


def _samples(n=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(1, 3, 64, 64, generator=g), torch.rand(1, 1, 8, 8, generator=g)) for _ in range(n)]


def test_parser_accum_and_clip_flags():
    import train
    p = train.build_parser()
    d = p.parse_args([])
    assert (d.accum_steps, d.clip_grad_norm) == (1, 0.0)
    a = p.parse_args(["--accum-steps", "4", "--clip-grad-norm", "2.5"])
    assert (a.accum_steps, a.clip_grad_norm) == (4, 2.5)
    assert p.parse_args(["--clip-grad-norm", "inf"]).clip_grad_norm == float("inf")
    with pytest.raises(SystemExit):
        p.parse_args(["--accum-steps", "0"])


def test_torch_stepper_window_is_one_batch2_step():
    """TorchStepper, fp32 CPU, k = 2 over two 1x3x64x64 samples: nothing moves and step() returns None on the first
    call; after the window every parameter's .grad is the gradient of ONE batch-2 step (the sum-reduced loss: no 1/k).

    Tolerance: per parameter, ||g_window - g_batch2|| / ||g_batch2||.  Measured on the development CPU against the
    batch-2 TorchStepper of the code before this feature (the k = 1 path, unchanged): largest value 1.4e-6 (1.39e-6 at
    1 thread, 1.07e-6 at 4, 0.95e-6 at 16; the batch-2 convolution sums the two samples inside one GEMM, the window
    adds two GEMM results).  Allowed: 10x that for thread-count dependence = 1.4e-5."""
    from can_distributed_pytorch_amd.engine.trainer import TorchStepper
    (xa, ga), (xb, gb) = _samples()
    m = _model()
    init = [p.detach().clone() for p in m.parameters()]
    st = TorchStepper("cpu", lr=1e-6, model=m, accum_steps=2)
    assert st.step(xa, ga) is None
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), init))
    loss = st.step(xb, gb)
    assert loss is not None and not all(torch.equal(p, q) for p, q in zip(m.parameters(), init))
    ref = TorchStepper("cpu", lr=1e-6, model=_model())
    loss2 = ref.step(torch.cat([xa, xb]), torch.cat([ga, gb]))
    assert torch.allclose(loss, loss2, rtol=1e-5)
    worst = 0.0
    for (n, p), q in zip(m.named_parameters(), ref.model.parameters()):
        rel = float((p.grad - q.grad).norm() / q.grad.norm())
        worst = max(worst, rel)
        assert rel <= 1.4e-5, (n, rel)
    print(f"largest relative-norm difference window vs batch 2: {worst:.3e}")


@pytest.mark.parametrize("name", ["sgd", "adamw"])
def test_arena_stepper_matches_torch_stepper_with_window_and_clipping(name):
    """ArenaStepper == TorchStepper over two windows of k = 2 with clip_grad_norm = 1 (the clip engages: the early
    gradient norm of the sum-reduced loss is far above 1), to the tolerance tests/test_optimizers.py holds the arena
    stepper to against torch.optim.  As there, the torch side's closing tail (clip_grad_norm_ + torch.optim) is fed the
    arena stepper's own accumulated gradients: Adam normalises the gradient magnitude away, so two backward passes
    that round a near-zero gradient to opposite signs differ by a full lr."""
    from can_distributed_pytorch_amd.engine.trainer import ArenaStepper, TorchStepper
    lr = 1e-4
    kw = dict(lr=lr, optimizer=name, weight_decay=5e-4, accum_steps=2, clip_grad_norm=1.0)
    a = ArenaStepper("cpu", model=_model(), **kw)
    t = TorchStepper("cpu", model=_model(), **kw)
    data = _samples(4)
    for w in range(2):
        (x0, g0), (x1, g1) = data[2 * w], data[2 * w + 1]
        assert a.step(x0, g0) is None and t.step(x0, g0) is None          # the window opens on both
        la = a.step(x1, g1)
        assert la is not None and t._micro == 1
        for p, q in zip(a.model.parameters(), t.model.parameters()):
            q.grad = p.grad.detach().clone()
        t._acc = la.reshape(()).clone()
        lt = t._finish_window()
        assert t._micro == 0 and float(lt) == float(la)
        assert a.clip_coef() < 1.0 and abs(a.grad_norm() - t.grad_norm()) <= 1e-5 * t.grad_norm()
    moved = 0.0
    for (n, p), q, p0 in zip(a.model.named_parameters(), t.model.parameters(), _model().parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6 * lr), (n, float((p - q).abs().max()))
        moved = max(moved, float((p.detach() - p0.detach()).abs().max()))
    assert moved > 0
    if name != "sgd":
        assert a.opt_steps == 2


def test_clipping_geometry_arena_stepper():
    """clip_grad_norm = 1e30 is bitwise the unclipped step; with a small max_norm the first SGD step (momentum 0)
    moves the arena by lr * max_norm in 2-norm."""
    from can_distributed_pytorch_amd.engine.trainer import ArenaStepper
    (x, g), = _samples(1)
    off = ArenaStepper("cpu", lr=1e-6, model=_model())
    big = ArenaStepper("cpu", lr=1e-6, model=_model(), clip_grad_norm=1e30)
    for _ in range(2):
        off.step(x, g)
        # the same gradient bits for both (two CPU backward passes need not agree bitwise across thread schedules)
        big.arena.grad.copy_(off.arena.grad)
        big._update()
    assert torch.equal(off.arena.data, big.arena.data) and torch.equal(off.mom, big.mom)
    assert not torch.equal(off.arena.data, ArenaStepper("cpu", model=_model()).arena.data)
    assert big.clip_coef() == 1.0
    lr, max_norm = 1e-2, 0.5
    st = ArenaStepper("cpu", lr=lr, momentum=0.0, model=_model(), clip_grad_norm=max_norm)
    before = st.arena.data.clone()
    st.step(x, g)
    assert st.grad_norm() > 100 * max_norm
    moved = float((st.arena.data.double() - before.double()).norm())
    assert abs(moved - lr * max_norm) <= 1e-5 * lr * max_norm, (moved, lr * max_norm)


def test_epoch_loop_flushes_the_open_window():
    """Three batches with k = 2: two optimizer steps, the second closing the one-batch window at the epoch's end."""
    from can_distributed_pytorch_amd.engine.train_eval import train_one_epoch
    m = _model()
    opt = torch.optim.SGD(m.parameters(), lr=1e-7, momentum=0.95)
    calls = []
    inner = opt.step
    opt.step = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    loader = [(x[0:1], g[0:1]) for x, g in _samples(3)]
    ml = train_one_epoch(m, opt, loader, "cpu", 0, accum_steps=2, clip_grad_norm=1.0)
    assert len(calls) == 2 and ml == ml
    # the same through a loader without a length (the flush after the loop)
    calls.clear()
    train_one_epoch(m, opt, iter(loader), "cpu", 0, accum_steps=2)
    assert len(calls) == 2


class _StubStepper:
    clip_grad_norm = 0.0

    def __init__(self):
        self.model = torch.nn.Linear(1, 1)
        self.calls = 0

    def reset_nonfinite(self):
        pass

    def nonfinite(self):
        return False

    def step(self, img, gt):
        self.calls += 1
        return None if self.calls % 2 else torch.tensor([2.0])

    def flush(self):
        return torch.tensor([1.0]) if self.calls % 2 else None


class _StubPrep:
    def issue(self, batch):
        return batch

    def ready(self, pending):
        return pending


@pytest.mark.parametrize("ahead", [False, True])
def test_native_epoch_loop_empty_loader_and_none_returns(ahead):
    from can_distributed_pytorch_amd.engine.train_eval import train_one_epoch_native
    prep = _StubPrep() if ahead else None
    st = _StubStepper()
    assert train_one_epoch_native(st, [], "cpu", 0, prep=prep) == 0.0 and st.calls == 0
    # three micro-batches, k = 2: window losses 2.0 (closing call) + 1.0 (flush) over 3 micro-batches
    batch = (torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 1, 1))
    assert train_one_epoch_native(st, [batch] * 3, "cpu", 0, prep=prep) == pytest.approx(1.0)


# ---------------------------------------------------------------- two gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _entry(rank, fn, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        fn(rank, world)
    finally:
        dist.destroy_process_group()


def _window_case(rank, world):
    from can_distributed_pytorch_amd.engine.trainer import ArenaStepper
    torch.set_num_threads(2)
    st = ArenaStepper("cpu", world=world, lr=1e-4, model=_model(rank), bucket_mb=4.0, accum_steps=2,
                      clip_grad_norm=1.0)
    launched = []
    inner = st.reducer._launch
    st.reducer._launch = lambda b: (launched.append(b), inner(b))[1]
    init = st.arena.data.clone()
    for i, (x, g) in enumerate(_samples(4, seed=10 + rank)):
        out = st.step(x, g)
        assert (out is None) == (i % 2 == 0)
        if i == 0:
            assert launched == [] and torch.equal(st.arena.data, init)       # paused: the hooks launched nothing
    nb = len(st.reducer.buckets)
    assert nb > 1 and launched == list(range(nb)) * 2                       # once per window
    assert not torch.equal(st.arena.data, init) and st.clip_coef() < 1.0
    ref = st.arena.data.clone()
    dist.broadcast(ref, src=0)
    assert torch.equal(ref, st.arena.data)


def test_arena_stepper_window_two_gloo_ranks():
    mp.spawn(_entry, args=(_window_case, 2, _free_port()), nprocs=2, join=True)


def test_train_py_torch_accum_clip_smoke(tmp_path):
    ck = tmp_path / "ck"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "64x64", "--synthetic-n", "6", "--epochs", "1",
           "--impl", "torch", "--device", "cpu", "--accum-steps", "2", "--clip-grad-norm", "1.0", "--num-workers", "0",
           "--wandb", "false", "--show", "false", "--checkpoint-dir", str(ck), "--log-jsonl", str(ck / "metrics.jsonl")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = [json.loads(x) for x in open(ck / "metrics.jsonl")]
    ep = [x for x in recs if x["kind"] == "epoch"]
    assert len(ep) == 1 and all(x["loss"] == x["loss"] and abs(x["loss"]) != float("inf") for x in ep)
