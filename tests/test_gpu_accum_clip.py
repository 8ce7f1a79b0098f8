"""Gradient accumulation and global-norm clipping on the GPU: the gradient-norm kernels (elementwise.hip
grad_norm_partial_kernel / grad_norm_final_kernel) against float64 torch, the optimizer kernels' device gradient
multiplier, the accumulation tick, and the NativeStepper's windows: arithmetic, bookkeeping, captured replay, fp16
overflow, a non-finite loss, and train.py end to end.  Everything runs at batch 1 on 64x64 and 96x128 inputs."""
import copy
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _C():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _model(seed=0):
    from can_distributed_pytorch_amd.models import CANNet
    torch.manual_seed(seed)
    m = CANNet(backend="torch")
    # He init so the signal survives 16 ReLU layers in a short test
    for mod in m.modules():
        if isinstance(mod, torch.nn.Conv2d):
            fan_in = mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1]
            torch.nn.init.normal_(mod.weight, std=(2.0 / fan_in) ** 0.5)
            if mod.bias is not None:
                torch.nn.init.uniform_(mod.bias, -0.05, 0.05)
    m.exec_backend = "hip"
    return m.cuda()


def _stepper(model, **kw):
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    kw.setdefault("graph", False)
    kw.setdefault("lr", 1e-7)
    return NativeStepper("cuda", model=copy.deepcopy(model), **kw)


def _batch(h, w, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(1, 3, h, w, device="cuda", generator=g),
            torch.rand(1, 1, h // 8, w // 8, device="cuda", generator=g))


def _within_2ulp(got: torch.Tensor, ref64: torch.Tensor):
    """|got - ref| <= 2 ulp of the fp32 rounding of the float64 value."""
    r32 = ref64.float()
    ulp = (torch.nextafter(r32, torch.full_like(r32, INF)) - r32).double()
    return bool(((got.double() - ref64).abs() <= 2 * ulp).all())


# ---------------------------------------------------------------- norm kernel
def _flat_norm(x, gscale=1.0, max_norm=INF, flags=None):
    C = _C()
    n = x.numel()
    tab = torch.tensor([[0, n]], dtype=torch.int64, device="cuda")
    part = torch.zeros(max(1, -(-n // C.grad_norm_chunk())), dtype=torch.float64, device="cuda")
    gn = torch.full((3,), -1.0, device="cuda")
    C.grad_norm(x.data_ptr(), tab.data_ptr(), 1, n, part.data_ptr(), gn.data_ptr(), gscale, max_norm,
                flags.data_ptr() + 8 if flags is not None else 0, _stream())
    torch.cuda.synchronize()
    return gn


@pytest.mark.parametrize("n", [1, 3, 4, 255, 4096, 4097, 3 * 4096 + 5])
def test_grad_norm_flat_vectors_against_float64(n):
    """One parameter of n elements from a 16-byte-aligned pointer (16-byte loads + tail) and from one float past it
    (element-wise path): global and per-parameter norm within 2 ulp of the fp32 rounding of the float64 value, two
    runs bitwise equal, max_norm = inf gives coefficient exactly 1, a finite max_norm torch's rule."""
    gen = torch.Generator(device="cuda").manual_seed(n)
    for mis in (0, 1):
        buf = torch.zeros(n + 8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        x = buf[mis:mis + n]
        x.copy_(torch.randn(n, device="cuda", generator=gen) *
                10.0 ** torch.randint(-3, 3, (n,), device="cuda", generator=gen).float())
        ref = x.double().pow(2).sum().sqrt()
        flags = torch.zeros(4, device="cuda")
        gn = _flat_norm(x, flags=flags)
        assert _within_2ulp(gn[0], ref) and _within_2ulp(gn[2], ref), (n, mis, float(gn[0]), float(ref))
        assert float(gn[1]) == 1.0 and float(flags[2]) == 0.0
        assert torch.equal(gn, _flat_norm(x, flags=flags))
        half = _flat_norm(x, gscale=0.5, max_norm=0.25 * float(ref))
        assert _within_2ulp(half[0], 0.5 * ref)
        want = min(1.0, np.float32(0.25 * float(ref)) / (np.float32(half[0].item()) + np.float32(1e-6)))
        assert abs(float(half[1]) - float(want)) <= 1e-6 * float(want) and float(half[1]) < 1.0


def test_grad_norm_model_arena_and_nonfinite():
    """The real model's gradient arena with random gradients (padding between the slots filled too: it must not
    count): the global norm and every per-parameter norm against float64, bitwise repeatable; one inf or one NaN
    element sets flags[2] and gives coefficient 0."""
    st = _stepper(_model(1), clip_grad_norm=INF)
    g = st.arena.grad
    g.copy_(torch.randn(g.numel(), device="cuda") * 3.0)
    views = st.arena.grad_views()
    per = torch.stack([v.double().pow(2).sum() for v in views])
    st.flags.zero_()
    gn = st.ex.grad_norm(1.0, INF, st.flags).clone()
    torch.cuda.synchronize()
    assert _within_2ulp(gn[0], per.sum().sqrt()), (float(gn[0]), float(per.sum().sqrt()))
    order = list(st.arena.order)
    assert _within_2ulp(gn[2:], per[order].sqrt())
    assert float(gn[1]) == 1.0 and float(st.flags[2]) == 0.0
    assert torch.equal(gn, st.ex.grad_norm(1.0, INF, st.flags))
    names = [n for n, _ in st.model.named_parameters()]
    norms = st.grad_norms()
    assert list(norms) == [names[i] for i in order] and st.grad_norm() == float(gn[0]) and st.clip_coef() == 1.0
    assert norms[names[order[3]]] == float(gn[2 + 3])
    o, cnt = st.arena.offsets[order[5]]
    for bad in (INF, float("nan")):
        keep = float(g[o + cnt - 1])
        g[o + cnt - 1] = bad
        st.flags.zero_()
        out = st.ex.grad_norm(1.0, 1.0, st.flags)
        torch.cuda.synchronize()
        assert float(st.flags[2]) == 1.0 and float(out[1]) == 0.0 and not math.isfinite(float(out[0]))
        g[o + cnt - 1] = keep
    st.flags.zero_()
    assert torch.equal(gn, st.ex.grad_norm(1.0, INF, st.flags)) and float(st.flags[2]) == 0.0


def test_accum_tick_folds_the_window_loss():
    C = _C()
    flags = torch.zeros(4, device="cuda")
    acc = torch.full((1,), 99.0, device="cuda")
    for i, (loss, fold, close) in enumerate([(1.5, 1, 0), (2.25, 2, 0), (4.0, 2, 1)]):
        flags[1] = loss
        flags[0] = 1.0
        C.accum_tick(flags.data_ptr(), acc.data_ptr(), fold, close, _stream())
    torch.cuda.synchronize()
    assert flags.tolist() == [0.0, 7.75, 0.0, 0.0] and float(acc) == 7.75
    flags[1] = float("nan")
    C.accum_tick(flags.data_ptr(), acc.data_ptr(), 2, 0, _stream())
    flags[1] = 1.0
    C.accum_tick(flags.data_ptr(), acc.data_ptr(), 0, 1, _stream())       # flush: nothing folded, the total written
    torch.cuda.synchronize()
    assert float(flags[0]) == 1.0 and math.isnan(float(flags[1]))


# ---------------------------------------------------------------- gmul
COEF, GS = 0.37, 0.5
HOST_GS = float(np.float32(GS) * np.float32(COEF))


@pytest.mark.parametrize("mis", [0, 1])
@pytest.mark.parametrize("decoupled,wd", [(0, 0.0), (1, 1e-2)])
def test_gmul_standalone_adam(decoupled, wd, mis):
    """C.adam with the device coefficient c == C.adam with float32(gscale) * float32(c) as gscale, bit for bit."""
    C = _C()
    n = 4099
    gen = torch.Generator(device="cuda").manual_seed(5)
    src = [torch.randn(n, device="cuda", generator=gen) for _ in range(4)]
    src[2].abs_()
    c = torch.tensor([COEF], device="cuda")
    out = []
    for gs, gm in ((GS, c.data_ptr()), (HOST_GS, 0)):
        bufs = [torch.zeros(n + 8, device="cuda") for _ in range(4)]
        p, m, v, g = (b[mis:mis + n] for b in bufs)
        for dst, s in zip((p, m, v, g), src):
            dst.copy_(s)
        C.adam(p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, wd, decoupled, gs, 3,
               0, 0, 0, _stream(), gm)
        torch.cuda.synchronize()
        out.append((p.clone(), m.clone(), v.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*out)) and not torch.equal(out[0][0], src[0])
    # and the multiplier really entered
    p, m, v, g = (s.clone() for s in src)
    C.adam(p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, wd, decoupled, GS, 3, 0,
           0, 0, _stream())
    torch.cuda.synchronize()
    assert not torch.equal(m, out[0][1])


def test_gmul_standalone_sgd_momentum():
    C = _C()
    n = 4096 + 4
    gen = torch.Generator(device="cuda").manual_seed(6)
    src = [torch.randn(n, device="cuda", generator=gen) for _ in range(3)]
    c = torch.tensor([COEF], device="cuda")
    out = []
    for gs, gm in ((GS, c.data_ptr()), (HOST_GS, 0), (GS, 0)):
        p, b, g = (s.clone() for s in src)
        C.sgd_momentum(p.data_ptr(), b.data_ptr(), g.data_ptr(), n, 1e-2, 0.95, gs, 0, 0, 0, _stream(), gm)
        torch.cuda.synchronize()
        out.append((p, b))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert not torch.equal(out[0][1], out[2][1])


def _arena(layout):
    """A full CANNet whose parameters are views of a flat master arena, gradient / first / second-moment arenas carved
    from the same buffer; 'aligned' or 'offset1' (every arena one float past 16-byte alignment: element-wise paths)."""
    from can_distributed_pytorch_amd.models import CANNet
    torch.manual_seed(9)
    model = CANNet().cuda()
    ps = list(model.parameters())
    k = sum(p.numel() for p in ps)
    pad = -(-k // 4) * 4 + 8
    big = torch.zeros(4 * pad + 8, device="cuda")
    assert big.data_ptr() % 16 == 0
    o = 1 if layout == "offset1" else 0
    data, grad, mom, mom2 = (big[s * pad + o:s * pad + o + k] for s in range(4))
    off = 0
    with torch.no_grad():
        for p in ps:
            c = p.numel()
            data[off:off + c].copy_(torch.randn(c, device="cuda") * 0.3)
            p.data = data[off:off + c].view_as(p)
            off += c
        grad.copy_(torch.randn(k, device="cuda"))
        mom.copy_(torch.randn(k, device="cuda"))
        mom2.copy_(torch.rand(k, device="cuda"))
    return model, big, data, grad, mom, mom2


def _snapshot(ex):
    packs = [t.clone() for s in ex.front + ex.back for t in ex.packs[id(s.module.weight)] if t is not None]
    packs += [t.clone() for sc in (1, 2, 3, 6) for t in ex.packs[id(ex.ctx2[sc].weight)]]
    return [ex.ctx2cat_fwd.clone(), ex.ctx2cat_dgr.clone()] + packs


@pytest.mark.parametrize("layout", ["aligned", "offset1"])
def test_gmul_fused_optimizers(layout):
    """executor.opt_step for SGD, SGD + weight decay, Adam and AdamW: the device coefficient == the host product as
    gscale, bit for bit over the masters, the moments, the step count and every 16-bit pack."""
    from can_distributed_pytorch_amd.ops.executor import CANNetExecutor
    model, big, data, grad, mom, mom2 = _arena(layout)
    ex = CANNetExecutor(model, dtype=torch.bfloat16)
    ex.refresh_packs(force=True)
    big0 = big.clone()
    c = torch.tensor([COEF], device="cuda")
    for hp in (dict(optimizer="sgd", weight_decay=0.0), dict(optimizer="sgd", weight_decay=5e-4),
               dict(optimizer="adam", weight_decay=0.0), dict(optimizer="adamw", weight_decay=1e-2)):
        res = []
        for gs, gm in ((GS, c), (HOST_GS, None), (GS, None)):
            with torch.no_grad():
                big.copy_(big0)
            ex.refresh_packs(force=True)
            t = torch.full((1,), 4, dtype=torch.int32, device="cuda")
            ex.opt_step(data, grad, mom, 3e-3, gs, momentum=0.95, mom2=mom2, step=t, gmul=gm, **hp)
            torch.cuda.synchronize()
            res.append((big.clone(), _snapshot(ex), int(t)))
        dev, host, plain = res
        assert torch.equal(dev[0], host[0]), (hp, float((dev[0] - host[0]).abs().max()))
        assert all(torch.equal(a, b) for a, b in zip(dev[1], host[1])) and dev[2] == host[2]
        assert not torch.equal(dev[0], plain[0]) and not torch.equal(dev[0], big0)


# ---------------------------------------------------------------- stepper: clipping
@pytest.mark.parametrize("name,lr,wd", [("sgd", 1e-2, 0.0), ("adamw", 1e-4, 1e-2)])
def test_stepper_clipping_matches_torch_clip_and_optim(name, lr, wd):
    """One bf16 step with clip_grad_norm = 1 (the clip engages): torch's clip_grad_norm_ + torch.optim in float64 on
    the step's own arena gradient, applied to the initial weights; the native arena's error against it is at most 4x
    that of fp32 torch.optim on the same inputs (the rule of tests/test_gpu_optimizers.py)."""
    model = _model(2)
    st = _stepper(model, lr=lr, optimizer=name, weight_decay=wd, momentum=0.95, clip_grad_norm=1.0)
    p0 = st.arena.data.clone()
    x, gt = _batch(64, 64, 1)
    st.step(x, gt)
    torch.cuda.synchronize()
    g = st.arena.grad.clone()
    assert not st.skipped_last() and st.grad_norm() > 1.0 and 0.0 < st.clip_coef() < 1.0

    def reference(dtype):
        q = p0.to(dtype).clone().requires_grad_(True)
        q.grad = g.to(dtype).clone()
        torch.nn.utils.clip_grad_norm_([q], 1.0)
        if name == "sgd":
            opt = torch.optim.SGD([q], lr=lr, momentum=0.95, weight_decay=wd, foreach=False)
        else:
            opt = torch.optim.AdamW([q], lr=lr, weight_decay=wd, foreach=False)
        opt.step()
        return q.detach()
    r64 = reference(torch.float64)
    e_native = float((st.arena.data.double() - r64).abs().max())
    e_torch = float((reference(torch.float32).double() - r64).abs().max())
    print(f"{name}: native {e_native:.3e}  torch fp32 {e_torch:.3e}  moved {float((r64 - p0.double()).abs().max()):.3e}")
    assert float((r64 - p0.double()).abs().max()) > 0
    assert e_native <= 4 * e_torch, (e_native, e_torch)


@pytest.mark.parametrize("name", ["sgd", "adamw"])
def test_stepper_huge_max_norm_is_bitwise_unclipped(name):
    model = _model(3)
    a = _stepper(model, optimizer=name, lr=1e-5)
    b = _stepper(model, optimizer=name, lr=1e-5, clip_grad_norm=1e30)
    x, gt = _batch(64, 64, 2)
    for _ in range(3):
        a.step(x, gt)
        b.step(x, gt)
    torch.cuda.synchronize()
    assert torch.equal(a.arena.data, b.arena.data) and torch.equal(a.mom, b.mom)
    assert b.clip_coef() == 1.0 and b.grad_norm() > 0 and a.grad_norm() is None
    assert not torch.equal(a.arena.data, _stepper(model).arena.data)


# ---------------------------------------------------------------- stepper: accumulation
def _pack(st):
    return st.ex.packs[id(st.ex.front[1].module.weight)][0]


def test_accumulation_arithmetic_and_open_window():
    """gAB (the arena after the open window A, B; A 64x64, B 96x128) against gA + gB of the micro-batches alone:
    elementwise |gAB - (gA + gB)| <= 4 * 2^-23 * (|gA| + |gB|) -- the accumulating kernels add the fresh sum to the
    previous value in fp32, possibly reassociated over a handful of launches.  While the window is open nothing but
    the gradient arena moves."""
    model = _model(4)
    A, B = _batch(64, 64, 3), _batch(96, 128, 4)
    alone = []
    for batch in (A, B):
        s = _stepper(model, accum_steps=2)
        assert s.step(*batch) is None
        torch.cuda.synchronize()
        alone.append(s.arena.grad.clone())
    gA, gB = alone
    st = _stepper(model, accum_steps=2)
    st.ex.refresh_packs()
    init = (st.arena.data.clone(), st.mom.clone(), _pack(st).clone())
    assert st.step(*A) is None
    torch.cuda.synchronize()
    assert torch.equal(st.arena.grad, gA)
    assert torch.equal(st.arena.data, init[0]) and torch.equal(st.mom, init[1]) and torch.equal(_pack(st), init[2])
    loss = st.step(*B)
    torch.cuda.synchronize()
    gAB = st.arena.grad.clone()
    bound = 4 * 2.0 ** -23 * (gA.abs() + gB.abs())
    err = (gAB - (gA + gB)).abs()
    print(f"max err / bound: {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    assert float(gA.abs().max()) > 0 and float(gB.abs().max()) > 0 and not torch.equal(gAB, gB)
    assert not torch.equal(st.arena.data, init[0]) and not torch.equal(st.mom, init[1])
    assert not torch.equal(_pack(st), init[2])
    # the window's loss is the sum of the micro-batch losses
    la = _stepper(model).step(*A)
    lb = _stepper(model).step(*B)
    assert abs(float(loss) - (float(la) + float(lb))) <= 1e-5 * (float(la) + float(lb))


def test_window_bookkeeping_and_flush():
    model = _model(5)
    st = _stepper(model, accum_steps=3, optimizer="adam", lr=1e-5)
    p0 = st.arena.data.clone()
    A, B = _batch(64, 64, 5), _batch(96, 128, 6)
    assert st.step(*A) is None and st.step(*B) is None
    assert int(st.opt_t) == 0 and torch.equal(st.arena.data, p0)
    loss = st.flush()
    torch.cuda.synchronize()
    assert loss is not None and math.isfinite(float(loss)) and int(st.opt_t) == 1
    assert not torch.equal(st.arena.data, p0) and not st.skipped_last()
    assert st.flush() is None and int(st.opt_t) == 1
    # the flushed window is the two-micro-batch window of a k = 2 stepper, bit for bit
    ref = _stepper(model, accum_steps=2, optimizer="adam", lr=1e-5)
    ref.step(*A)
    loss2 = ref.step(*B)
    torch.cuda.synchronize()
    assert torch.equal(st.arena.data, ref.arena.data) and float(loss) == float(loss2)
    # and the next window starts fresh
    assert st.step(*A) is None


@pytest.mark.parametrize("transport", [None, "rccl"])
@pytest.mark.parametrize("k", [2, 3])
def test_captured_windows_replay_the_eager_ones_bitwise(k, transport):
    """From a cold stepper with graph=True: three windows of k micro-steps equal graph=False bit for bit, with one
    capture per phase of the shape (a capture's warm-up must neither clobber the open window nor add into it)."""
    model = _model(6)
    kw = dict(accum_steps=k, clip_grad_norm=5.0, lr=1e-6)
    if transport:
        kw.update(reducer_transport=transport, bucket_mb=4.0)
    a = _stepper(model, graph=False, **kw)
    b = _stepper(model, graph=True, **kw)
    for i in range(3 * k):
        x, gt = _batch(64, 64, 100 + i)
        la, lb = a.step(x, gt), b.step(x, gt)
        assert (la is None) == (lb is None) == ((i + 1) % k != 0)
        if la is not None:
            assert float(la) == float(lb)
    torch.cuda.synchronize()
    assert b.graph_captures == k
    assert torch.equal(a.arena.data, b.arena.data) and torch.equal(a.mom, b.mom)
    assert torch.equal(a.arena.grad, b.arena.grad) and a.grad_norm() == b.grad_norm()
    assert not torch.equal(a.arena.data, _stepper(model).arena.data)


def test_captured_windows_mixed_shapes():
    """A (96x128) always opens, B (64x64) always closes: B is first met inside an open window, so that occurrence runs
    eagerly as the real micro-step and the next one is captured (B is the smaller shape: the shared weight-gradient
    workspace does not grow, which would drop A's graph)."""
    model = _model(7)
    a = _stepper(model, graph=False, accum_steps=2, lr=1e-6)
    b = _stepper(model, graph=True, accum_steps=2, lr=1e-6)
    for i in range(3):
        for h, w in ((96, 128), (64, 64)):
            x, gt = _batch(h, w, 200 + 2 * i + h)
            a.step(x, gt)
            b.step(x, gt)
    torch.cuda.synchronize()
    assert b.graph_captures == 2
    assert torch.equal(a.arena.data, b.arena.data) and torch.equal(a.mom, b.mom)


@pytest.mark.parametrize("clip", [0.0, 1.0])
def test_fp16_overflow_skips_the_whole_window(clip):
    """fp16 from a loss scale of 2^40: every micro-step overflows; the window is skipped, the arena untouched and the
    scale halved once per window, not per micro-step; a later window at a sane scale applies.  With clipping on the
    norm pass is the overflow check."""
    st = _stepper(_model(8), dtype="fp16", init_scale=2.0 ** 40, scale_interval=10 ** 6, accum_steps=2, lr=1e-6,
                  clip_grad_norm=clip)
    p0 = st.arena.data.clone()
    A, B = _batch(64, 64, 7), _batch(96, 128, 8)
    for w in range(2):
        assert st.step(*A) is None
        assert st.loss_scale() == 2.0 ** (40 - w)
        st.step(*B)
        assert st.skipped_last() and st.loss_scale() == 2.0 ** (39 - w)
    assert torch.equal(st.arena.data, p0) and not st.nonfinite()
    st.scaler.copy_(torch.tensor([64.0, 1.0 / 64.0, 0.0, 0.0], device="cuda"))
    st.step(*A)
    st.step(*B)
    assert not st.skipped_last() and st.loss_scale() == 64.0 and not torch.equal(st.arena.data, p0)


def test_nonfinite_loss_in_one_micro_batch_skips_the_window():
    st = _stepper(_model(9), accum_steps=2, lr=1e-6, clip_grad_norm=10.0)
    p0 = st.arena.data.clone()
    A, B = _batch(64, 64, 9), _batch(96, 128, 10)
    bad = A[1].clone()
    bad[0, 0, 0, 0] = float("nan")
    st.step(A[0], bad)
    loss = st.step(*B)
    assert math.isnan(float(loss)) and st.skipped_last() and st.nonfinite()
    assert torch.equal(st.arena.data, p0) and float(st.mom.abs().max()) == 0
    st.reset_nonfinite()
    st.step(*A)
    loss = st.step(*B)
    assert math.isfinite(float(loss)) and not st.skipped_last() and not st.nonfinite()
    assert not torch.equal(st.arena.data, p0)


def test_train_py_accum_clip_native(tmp_path):
    ck = tmp_path / "ck"
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "64x64", "--epochs", "1", "--accum-steps", "2",
           "--clip-grad-norm", "1.0", "--optimizer", "adamw", "--num-workers", "0", "--wandb", "false", "--show", "false",
           "--checkpoint-dir", str(ck), "--log-jsonl", str(ck / "metrics.jsonl")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    recs = [json.loads(x) for x in open(ck / "metrics.jsonl")]
    tr = [x for x in recs if x["kind"] == "train"]
    ep = [x for x in recs if x["kind"] == "epoch"]
    assert tr and all(np.isfinite(x["mean_loss"]) and x["grad_norm"] > 0 and 0 < x["clip_coef"] <= 1 for x in tr)
    assert len(ep) == 1 and np.isfinite(ep[0]["loss"])
