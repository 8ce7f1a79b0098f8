"""EMA of the weights on the CPU paths: the flags, the torch-op steppers' values against the float64 recurrence,
accumulation windows, the ``ema_weights()`` swap, train.py's checkpoints and resume, and two gloo ranks.

The bound: one update e += w (p - e) in fp32 is one subtraction and one multiply-add (torch may round the product
and the sum separately: three roundings of at most 2^-24 relative each, on magnitudes of at most 2A, A the running
max of |p| and |e|), and earlier errors are multiplied by d <= 1, so |e - e64| <= T * 2^-22 * A after T updates (the
GPU kernel's bound, tests/test_gpu_ema.py, which has one rounding fewer)."""
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


def _model(seed=0):
    from can_distributed_pytorch_amd.models import CANNet
    torch.manual_seed(seed)
    m = CANNet(backend="torch")
    for mod in m.modules():                       # He init: visible gradients in a few steps
        if isinstance(mod, torch.nn.Conv2d):
            torch.nn.init.normal_(mod.weight, std=(2.0 / (mod.in_channels * 9)) ** 0.5)
    return m


def _batch(step, n=2):
    g = torch.Generator().manual_seed(100 + step)
    return torch.randn(n, 3, 32, 32, generator=g), torch.rand(n, 1, 4, 4, generator=g)


def _stepper(kind, **kw):
    from can_distributed_pytorch_amd.engine.trainer import ArenaStepper, TorchStepper
    if kind == "torch":
        return TorchStepper("cpu", dtype="fp32", lr=1e-5, model=_model(), **kw)
    return ArenaStepper("cpu", lr=1e-5, model=_model(), **kw)


def _params(st):
    return [p.detach().clone() for p in st.model.parameters()]


def _ema_list(st):
    return list(st.ema_state()["ema"].values())


def _d(n, decay, warmup):
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


def _recurrence64(e0, weights, decay, warmup):
    """The float64 recurrence over recorded fp32 weights, with w = float32(1 - d_n) as every implementation uses it;
    returns the result and the running max A of |p|, |e| per element."""
    e = [x.double() for x in e0]
    A = [x.abs().double() for x in e0]
    for n, ps in enumerate(weights):
        w = float(torch.tensor(1.0 - _d(n, decay, warmup), dtype=torch.float64).float())
        for i, p in enumerate(ps):
            e[i] = e[i] + w * (p.double() - e[i])
            A[i] = torch.maximum(A[i], torch.maximum(p.abs().double(), e[i].abs()))
    return e, A


def test_parser_ema_flags():
    sys.path.insert(0, ROOT)
    import train
    p = train.build_parser()
    a = p.parse_args([])
    assert a.ema_decay == 0.0 and a.ema_warmup is True
    a = p.parse_args(["--ema-decay", "0.999", "--ema-warmup", "false"])
    assert a.ema_decay == 0.999 and a.ema_warmup is False
    for bad in ("-0.1", "1", "1.5", "nan"):
        with pytest.raises(SystemExit):
            p.parse_args(["--ema-decay", bad])


@pytest.mark.parametrize("kind", ["torch", "arena"])
def test_steppers_refuse_a_decay_outside_the_unit_interval(kind):
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            _stepper(kind, ema_decay=bad)
    st = _stepper(kind)                                        # off: no copies, no context manager
    assert st.ema_state() is None
    with pytest.raises(RuntimeError, match="off"):
        with st.ema_weights():
            pass


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("kind", ["torch", "arena"])
def test_stepper_ema_is_the_float64_recurrence(kind, warmup):
    T, decay = 5, 0.999
    st = _stepper(kind, ema_decay=decay, ema_warmup=warmup)
    e0 = _ema_list(st)
    assert all(torch.equal(a, b) for a, b in zip(e0, _params(st)))      # starts from the weights
    rec = []
    for s in range(T):
        st.step(*_batch(s))
        rec.append(_params(st))
        if s == 0:
            # the first update: d_0 = 0.1 with warm-up (w = 0.9), decay without
            w0 = float(torch.tensor(1.0 - (0.1 if warmup else decay), dtype=torch.float64).float())
            e1 = _ema_list(st)
            moved = False
            for a, b, c in zip(e0, rec[0], e1):
                want = a.double() + w0 * (b.double() - a.double())
                assert float((c.double() - want).abs().max()) <= 2.0 ** -22 * float(torch.maximum(a.abs(), b.abs()).max())
                moved = moved or not torch.equal(a, b)
            assert moved
    assert st.ema_state()["steps"] == T
    ref, A = _recurrence64(e0, rec, decay, warmup)
    worst = 0.0
    for e, r, a in zip(_ema_list(st), ref, A):
        err = (e.double() - r).abs()
        assert bool((err <= T * 2.0 ** -22 * a).all()), float((err / a.clamp_min(1e-30)).max())
        worst = max(worst, float((err / a.clamp_min(1e-30)).max()))
    print(f"{kind} warmup={warmup}: max |e - e64| / A = {worst:.3e} (bound {T * 2.0 ** -22:.3e})")
    # and the average is not the weights
    assert any(not torch.equal(e, p) for e, p in zip(_ema_list(st), _params(st)))


@pytest.mark.parametrize("kind", ["torch", "arena"])
def test_ema_updates_once_per_accumulation_window(kind):
    st = _stepper(kind, ema_decay=0.9, accum_steps=3)
    e0 = _ema_list(st)
    steps = []
    for s in range(7):
        out = st.step(*_batch(s, n=1))
        steps.append(st.ema_state()["steps"])
        same = all(torch.equal(a, b) for a, b in zip(e0, _ema_list(st)))
        if (s + 1) % 3:
            assert out is None and same, s
        else:
            assert out is not None and not same, s
            e0 = _ema_list(st)
    assert steps == [0, 0, 1, 1, 1, 2, 2]
    with pytest.raises(RuntimeError, match="window"):             # micro-step 7 opened a window
        with st.ema_weights():
            pass
    assert st.flush() is not None
    assert st.ema_state()["steps"] == 3
    assert not all(torch.equal(a, b) for a, b in zip(e0, _ema_list(st)))
    with st.ema_weights():
        pass


@pytest.mark.parametrize("kind", ["torch", "arena"])
def test_ema_weights_swaps_and_restores_bitwise(kind):
    st = _stepper(kind, ema_decay=0.9)
    for s in range(2):
        st.step(*_batch(s))
    raw, avg = _params(st), _ema_list(st)
    x = _batch(9)[0]
    st.model.eval()
    with torch.no_grad():
        y_raw = st.model(x)
    with st.ema_weights() as m:
        assert m is st.model
        assert all(torch.equal(p, e) for p, e in zip(st.model.parameters(), avg))
        assert all(torch.equal(v, e) for v, e in zip(st.model.state_dict().values(), avg))
        assert all(torch.equal(a, e) for a, e in zip(_ema_list(st), avg))       # ema_state: still the average
        with torch.no_grad():
            y_avg = st.model(x)
        with pytest.raises(RuntimeError, match="nest"):
            with st.ema_weights():
                pass
    assert not torch.equal(y_avg, y_raw)
    assert all(torch.equal(p, r) for p, r in zip(st.model.parameters(), raw))
    assert all(torch.equal(a, e) for a, e in zip(_ema_list(st), avg))
    with torch.no_grad():
        assert torch.equal(st.model(x), y_raw)


# ---------------------------------------------------------------- train.py
def _train(tmp, ck, *extra, epochs=2):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "32x48", "--synthetic-n", "6", "--epochs",
           str(epochs), "--impl", "torch", "--device", "cpu", "--num-workers", "0", "--wandb", "false", "--show",
           "false", "--lr", "1e-6", "--checkpoint-dir", str(ck), "--log-jsonl", str(ck / "metrics.jsonl"), *extra]
    env = dict(os.environ, OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp), env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def test_train_py_checkpoints_the_average_and_resumes_it(tmp_path):
    ema = ("--ema-decay", "0.9")
    a = tmp_path / "a"
    _train(tmp_path, a, *ema, epochs=3)                          # the uninterrupted run
    b = tmp_path / "b"
    _train(tmp_path, b, *ema, epochs=2)
    st = _load(b / "last_state.pth")
    assert st["ema_steps"] == 12 and st["ema_decay"] == 0.9
    assert set(st["ema"]) == {k for k in st["model"]}
    best = sorted(p for p in os.listdir(b) if p.startswith("epoch_"))[-1]
    sd = _load(b / best)
    assert any(not torch.equal(sd[k], st["model"][k]) for k in sd)          # not the raw weights
    assert any(not torch.equal(st["ema"][k], st["model"][k]) for k in st["model"])
    ep = [json.loads(x) for x in open(b / "metrics.jsonl")]
    assert all(x["ema_decay"] == 0.9 for x in ep if x["kind"] == "epoch")
    # resume: a third epoch equals the uninterrupted run's
    out = _train(tmp_path, b, *ema, "--resume", str(b / "last_state.pth"), epochs=3)
    assert "has no EMA" not in out
    sa, sb = _load(a / "last_state.pth"), _load(b / "last_state.pth")
    assert sa["ema_steps"] == sb["ema_steps"] == 18
    for k in sa["model"]:
        assert torch.equal(sa["model"][k], sb["model"][k]), k
        assert torch.equal(sa["ema"][k], sb["ema"][k]), k


def test_train_py_every_epoch_checkpoint_is_the_average(tmp_path):
    """One epoch: epoch_0.pth (always the best so far) holds exactly the average that last_state.pth carries."""
    c = tmp_path / "c"
    _train(tmp_path, c, "--ema-decay", "0.9", epochs=1)
    st, sd = _load(c / "last_state.pth"), _load(c / "epoch_0.pth")
    assert list(sd) == list(st["model"])
    assert all(torch.equal(sd[k], st["ema"][k]) for k in sd)
    assert any(not torch.equal(sd[k], st["model"][k]) for k in sd)


def test_train_py_resume_without_and_into_no_ema(tmp_path):
    d = tmp_path / "d"
    _train(tmp_path, d, epochs=1)
    st = _load(d / "last_state.pth")
    assert "ema" not in st and "ema_steps" not in st             # EMA off: the file of before
    out = _train(tmp_path, d, "--ema-decay", "0.9", "--resume", str(d / "last_state.pth"), epochs=2)
    assert "has no EMA; the average starts from the loaded weights at n = 0" in out
    st = _load(d / "last_state.pth")
    assert st["ema_steps"] == 6
    out = _train(tmp_path, d, "--resume", str(d / "last_state.pth"), epochs=3)
    assert "holds an EMA of the weights; ignored" in out


# ---------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _entry(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from can_distributed_pytorch_amd.engine.trainer import ArenaStepper
        torch.set_num_threads(2)
        st = ArenaStepper("cpu", world=world, lr=1e-5, model=_model(rank), bucket_mb=4.0, ema_decay=0.99)
        for s in range(3):
            st.step(*_batch(10 * rank + s, n=1))                # different data, different initial models
        es = st.ema_state()
        assert es["steps"] == 3
        mine = torch.cat([v.reshape(-1) for v in es["ema"].values()])
        ref = mine.clone()
        dist.broadcast(ref, src=0)
        assert torch.equal(ref, mine)
        assert float(mine.abs().max()) > 0
        raw = torch.cat([p.detach().reshape(-1) for p in st.model.parameters()])
        assert not torch.equal(raw, mine)
    finally:
        dist.destroy_process_group()


def test_arena_stepper_ema_is_replicated_on_two_gloo_ranks():
    mp.spawn(_entry, args=(2, _free_port()), nprocs=2, join=True)
