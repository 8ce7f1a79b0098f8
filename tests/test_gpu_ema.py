"""EMA of the weights on the GPU (elementwise.hip: ema_kernel, pack_multi_kernel<DT, OPT, EMA = true>, the OPT_SWAP
launch, opt_tick_kernel): values against the float64 recurrence, the skip flags, the fused launch against the
two-launch step bit for bit, the swap, the whole NativeStepper step, captured replay, evaluation under the averaged
weights, resume and the custom operator.

The bound of the value tests: one update e += w (p - e) is one fp32 subtraction (error <= 2^-24 * |p - e| <=
2^-23 * A) and one fma (error <= 2^-24 * |e'| <= 2^-24 * A), A the running max of |p| and |e| per element; earlier
errors are multiplied by d = 1 - w <= 1.  Hence |e - e64| <= T * 2^-22 * A after T updates (w itself is the same
float in the kernel and in the reference).  Numerics measured on an MI355X are recorded in
profiles/r11/ema_numerics.txt."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DECAY = 0.999
SIZES = (1, 3, 4, 5, 4099, 2 ** 20 + 1)


def _C():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _w(n, decay, warmup):
    d = min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay
    return float(torch.tensor(1.0 - d, dtype=torch.float64).float())


def _recurrence(e0, ps, decay, warmup, n0, dtype):
    """e_t in ``dtype`` over the recorded fp32 p_t (w = float32(1 - d_n) throughout); returns e and, per element, the
    running max A of |p|, |e|."""
    e = e0.to(dtype)
    A = e0.abs().double()
    for k, p in enumerate(ps):
        w = _w(n0 + k, decay, warmup)
        e = e + w * (p.to(dtype) - e)
        A = torch.maximum(A, torch.maximum(p.abs().double(), e.abs().double()))
    return e, A


def _native_ema(e0, ps, decay, warmup, n0, misalign):
    """C.ema over buffers whose base is 16-B aligned (misalign 0) or one float past it."""
    C = _C()
    n = e0.numel()
    bufs = [torch.zeros(n + 8, device="cuda") for _ in range(2)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    e, p = (b[misalign:misalign + n] for b in bufs)
    e.copy_(e0)
    t = torch.full((1,), n0, dtype=torch.int32, device="cuda")
    for pi in ps:
        p.copy_(pi)
        C.ema(e.data_ptr(), p.data_ptr(), n, decay, int(warmup), 0, t.data_ptr(), 0, _stream())
    torch.cuda.synchronize()
    assert int(t) == n0 + len(ps)
    assert torch.equal(p, ps[-1])
    for b in bufs:          # nothing written outside the span
        assert float(b[:misalign].abs().sum()) == 0 and float(b[misalign + n:].abs().sum()) == 0
    return e.clone()


def _ema_case(T, warmup, n0=0, sizes=SIZES):
    gen = torch.Generator(device="cuda").manual_seed(4321 + T + n0)
    for n in sizes:
        scale = 10.0 ** torch.randint(-4, 3, (n,), device="cuda", generator=gen).float()
        e0 = torch.randn(n, device="cuda", generator=gen) * scale
        ps = [torch.randn(n, device="cuda", generator=gen) * scale for _ in range(T)]
        ref, A = _recurrence(e0, ps, DECAY, warmup, n0, torch.float64)
        e32, _ = _recurrence(e0, ps, DECAY, warmup, n0, torch.float32)
        yard = float(((e32.double() - ref).abs() / A).max())
        for mis in (0, 1):
            got = _native_ema(e0, ps, DECAY, warmup, n0, mis)
            err = (got.double() - ref).abs() / A
            print(f"ema warmup={int(warmup)} T={T:2d} n0={n0:4d} n={n:7d} mis={mis} "
                  f"max|e-e64|/A {float(err.max()):.3e} (torch fp32 ops {yard:.3e}; bound {T * 2.0 ** -22:.3e})")
            assert float(err.max()) <= T * 2.0 ** -22, (T, warmup, n, mis, float(err.max()))
            assert not torch.equal(got, e0)


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("T", [1, 25])
def test_ema_kernel_values(T, warmup):
    """C.ema against the float64 recurrence over the same fp32 p_t: |e - e64| <= T * 2^-22 * A for every size, at
    16-byte alignment (float4 groups + tail) and one float off it (element-wise)."""
    _ema_case(T, warmup)


def test_ema_kernel_count_preset_to_1000():
    """ema_t = 1000: the warm-up term (1001 / 1010) is above the decay, d_n = decay."""
    _ema_case(3, True, n0=1000, sizes=(5, 4099))
    # and the first update with warm-up is d_0 = 0.1: e1 = e0 + 0.9 (p - e0) to rounding
    e0, p = torch.zeros(4099, device="cuda"), torch.ones(4099, device="cuda")
    got = _native_ema(e0, [p], DECAY, True, 0, 0)
    assert torch.equal(got, torch.full_like(got, float(torch.tensor(0.9, dtype=torch.float64).float())))
    got = _native_ema(e0, [p], DECAY, False, 0, 0)
    assert torch.equal(got, torch.full_like(got, float(torch.tensor(1.0 - DECAY, dtype=torch.float64).float())))


def test_ema_kernel_skip_flags_and_refusals():
    C = _C()
    n = 4099
    e, p = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
    t = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    before = e.clone()
    for idx in (0, 2):
        flags = torch.zeros(4, device="cuda")
        flags[idx] = 1.0
        C.ema(e.data_ptr(), p.data_ptr(), n, DECAY, 1, 0, t.data_ptr(), flags.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert torch.equal(e, before) and int(t) == 7
        assert float(flags[3]) == (1.0 if idx == 0 else 0.0)
    flags = torch.zeros(4, device="cuda")
    C.ema(e.data_ptr(), p.data_ptr(), n, DECAY, 1, 0, t.data_ptr(), flags.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert int(t) == 8 and not torch.equal(e, before)
    # the same update from the host's step (n = step - 1) is the device count's, bit for bit
    e2 = before.clone()
    C.ema(e2.data_ptr(), p.data_ptr(), n, DECAY, 1, 8, 0, 0, _stream())
    torch.cuda.synchronize()
    assert torch.equal(e, e2)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(RuntimeError):
            C.ema(e.data_ptr(), p.data_ptr(), n, bad, 1, 0, t.data_ptr(), 0, _stream())
    with pytest.raises(RuntimeError):                       # neither a device count nor a step
        C.ema(e.data_ptr(), p.data_ptr(), n, DECAY, 1, 0, 0, 0, _stream())


# ---------------------------------------------------------------- fused == two-launch
def _arena(layout):
    """A full CANNet whose parameters are views of a flat master arena, with gradient / first-moment / second-moment /
    EMA arenas carved from one buffer.  layout: 'aligned' (all 16-B aligned), 'offset1' (every arena one float past
    alignment: element-wise paths, offsets between the arenas still whole float4s) or 'e_mod4_1' (masters aligned, the
    EMA arena 1 (mod 4) floats from them: the v4 guard must send the step down the element-wise path).  The values do
    not depend on the layout."""
    from can_distributed_pytorch_amd.models import CANNet
    torch.manual_seed(9)
    model = CANNet().cuda()
    ps = list(model.parameters())
    k = sum(p.numel() for p in ps)
    pad = -(-k // 4) * 4 + 8
    big = torch.zeros(5 * pad + 8, device="cuda")
    assert big.data_ptr() % 16 == 0
    o = 1 if layout == "offset1" else 0
    starts = [o, pad + o, 2 * pad + o, 3 * pad + o, 4 * pad + o + (layout == "e_mod4_1")]
    data, grad, mom, mom2, ema = (big[s:s + k] for s in starts)
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
        ema.copy_(torch.randn(k, device="cuda") * 0.3)
    return model, big, data, grad, mom, mom2, ema


def _snapshot(ex):
    packs = [t.clone() for s in ex.front + ex.back for t in ex.packs[id(s.module.weight)] if t is not None]
    packs += [t.clone() for sc in (1, 2, 3, 6) for t in ex.packs[id(ex.ctx2[sc].weight)]]
    return [ex.ctx2cat_fwd.clone(), ex.ctx2cat_dgr.clone()] + packs


OPTS = {"sgd": dict(optimizer="sgd", momentum=0.95), "sgd_wd": dict(optimizer="sgd", momentum=0.95, weight_decay=5e-4),
        "adamw": dict(optimizer="adamw", weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8)}
N0 = 3          # the preset update count: warm-up gives d_3 = 4 / 13, so w is neither 0.9 nor 1 - decay


def _fused_run(layout, dtype, opt):
    """The fused step with EMA on a fresh arena of ``layout``; returns everything the comparisons need."""
    from can_distributed_pytorch_amd.engine.native import ACT_DTYPES
    from can_distributed_pytorch_amd.ops.executor import CANNetExecutor
    model, big, data, grad, mom, mom2, ema = _arena(layout)
    ex = CANNetExecutor(model, dtype=ACT_DTYPES[dtype])
    ex.refresh_packs(force=True)
    adam = opt == "adamw"
    flags = torch.zeros(4, device="cuda")
    lr_dev = torch.tensor([3e-3], device="cuda")
    t = torch.full((1,), 11, dtype=torch.int32, device="cuda") if adam else None
    et = torch.full((1,), N0, dtype=torch.int32, device="cuda")
    kw = dict(OPTS[opt], mom2=mom2 if adam else None, step=t, flags=flags, lr_dev=lr_dev)
    return dict(model=model, big=big, data=data, grad=grad, mom=mom, mom2=mom2, ema=ema, ex=ex, flags=flags, t=t,
                et=et, kw=kw, adam=adam)


_ALIGNED = {}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("layout", ["aligned", "offset1", "e_mod4_1"])
@pytest.mark.parametrize("opt", list(OPTS))
def test_fused_ema_matches_two_launch_step(opt, layout, dtype):
    """executor.opt_step(..., ema=) (optimizer + EMA + the 16-bit packs, one launch + the tick) == opt_step without
    EMA followed by C.ema over the arena, bit for bit: masters, momentum(s), e, every pack, the interleaved context
    packs, Adam's step count and the EMA's update count.  'e_mod4_1' takes the element-wise path and gives the
    aligned layout's result.  (For plain SGD the two-launch arm's opt_step is the default training step's launch,
    pack_multi_kernel<DT, OPT_SGD, false>: its masters, momentum and packs are compared there.)  Then the skip flags."""
    C = _C()
    r = _fused_run(layout, dtype, opt)
    ex, big, data, grad, mom, ema, flags, t, et, kw = (r[k] for k in ("ex", "big", "data", "grad", "mom", "ema",
                                                                      "flags", "t", "et", "kw"))
    big0, e_init = big.clone(), ema.clone()
    # two launches
    ex.opt_step(data, grad, mom, 1.0, 0.5, **kw)
    C.ema(ema.data_ptr(), data.data_ptr(), data.numel(), DECAY, 1, 0, et.data_ptr(), flags.data_ptr(), _stream())
    torch.cuda.synchronize()
    ref_big, ref_packs = big.clone(), _snapshot(ex)
    assert not torch.equal(data, big0[:data.numel()]) and not torch.equal(ema, e_init)
    assert int(et) == N0 + 1 and (t is None or int(t) == 12)
    # fused
    with torch.no_grad():
        big.copy_(big0)
    ex.refresh_packs(force=True)
    et.fill_(N0)
    if t is not None:
        t.fill_(11)
    ex.opt_step(data, grad, mom, 1.0, 0.5, ema=ema, ema_t=et, ema_decay=DECAY, ema_warmup=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(big, ref_big), float((big - ref_big).abs().max())
    assert int(et) == N0 + 1 and (t is None or int(t) == 12)
    got_packs = _snapshot(ex)
    for i, (g, q) in enumerate(zip(got_packs, ref_packs)):
        assert torch.equal(g, q), i
    state = [x.clone() for x in (data, mom, ema)] + ([r["mom2"].clone()] if r["adam"] else [])
    if layout == "aligned":
        _ALIGNED[(opt, dtype)] = (state, got_packs)
    # skip semantics
    before_big, before_packs = big.clone(), _snapshot(ex)
    for idx in (0, 2):
        flags.zero_()
        flags[idx] = 1.0
        ex.opt_step(data, grad, mom, 1.0, 0.5, ema=ema, ema_t=et, ema_decay=DECAY, ema_warmup=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(big, before_big) and int(et) == N0 + 1 and (t is None or int(t) == 12)
        assert all(torch.equal(a, b) for a, b in zip(_snapshot(ex), before_packs))
        assert float(flags[3]) == (1.0 if idx == 0 else 0.0)
    if layout == "e_mod4_1":
        del r, ex, big, data, grad, mom, ema
        if (opt, dtype) not in _ALIGNED:
            a = _fused_run("aligned", dtype, opt)
            a["ex"].opt_step(a["data"], a["grad"], a["mom"], 1.0, 0.5, ema=a["ema"], ema_t=a["et"], ema_decay=DECAY,
                             ema_warmup=True, **a["kw"])
            torch.cuda.synchronize()
            _ALIGNED[(opt, dtype)] = ([x.clone() for x in (a["data"], a["mom"], a["ema"])] +
                                      ([a["mom2"].clone()] if a["adam"] else []), _snapshot(a["ex"]))
        ref_state, ref_p = _ALIGNED[(opt, dtype)]
        for i, (g, q) in enumerate(zip(state, ref_state)):
            assert torch.equal(g, q), ("state", i)
        for i, (g, q) in enumerate(zip(got_packs, ref_p)):
            assert torch.equal(g, q), ("pack", i)


def test_opt_step_refuses_a_bad_ema_setup():
    r = _fused_run("aligned", "bf16", "sgd")
    ex, data, grad, mom, ema, et, kw = (r[k] for k in ("ex", "data", "grad", "mom", "ema", "et", "kw"))
    with pytest.raises(ValueError, match="ema_t"):
        ex.opt_step(data, grad, mom, 1.0, 0.5, ema=ema, ema_t=None, ema_decay=DECAY, **kw)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="ema_decay"):
            ex.opt_step(data, grad, mom, 1.0, 0.5, ema=ema, ema_t=et, ema_decay=bad, **kw)
    with pytest.raises(ValueError, match="EMA arena"):
        ex.opt_step(data, grad, mom, 1.0, 0.5, ema=ema[:-1], ema_t=et, ema_decay=DECAY, **kw)
    # the C entry point refuses on its own: a null count, a decay outside [0, 1)
    desc, rows, tiles, goff, boff, voff, eoff = ex.opt_prepare(data, grad, mom, None, ema)
    base = (desc, rows, tiles, 1, goff, boff, 0, 1e-3, 0.95, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, 0, 0, 0, ex.dt, _stream(), 0)
    for eargs in ((eoff, DECAY, 1, 0), (eoff, 1.0, 1, et.data_ptr()), (eoff, -0.5, 1, et.data_ptr())):
        with pytest.raises(RuntimeError):
            ex.C.opt_pack(*base, *eargs)


# ---------------------------------------------------------------- swap
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("layout", ["aligned", "offset1", "e_mod4_1"])
def test_swap_weights(layout, dtype):
    """After swap_weights the masters hold the old e and e the old masters; every pack and the interleaved context
    packs are refresh_packs(force=True) of those weights; a second swap restores everything bit for bit."""
    r = _fused_run(layout, dtype, "sgd")
    ex, big, data, grad, mom, ema = (r[k] for k in ("ex", "big", "data", "grad", "mom", "ema"))
    ex.opt_prepare(data, grad, mom, None, ema)
    torch.cuda.synchronize()
    big0, packs0 = big.clone(), _snapshot(ex)
    d0, e0, g0, m0 = data.clone(), ema.clone(), grad.clone(), mom.clone()
    r["flags"][0] = 1.0                                            # the swap ignores the step's flags
    ex.swap_weights(data, ema)
    torch.cuda.synchronize()
    assert torch.equal(data, e0) and torch.equal(ema, d0) and not torch.equal(d0, e0)
    assert torch.equal(grad, g0) and torch.equal(mom, m0)
    got = _snapshot(ex)
    ex.refresh_packs(force=True)
    torch.cuda.synchronize()
    for i, (g, q) in enumerate(zip(got, _snapshot(ex))):
        assert torch.equal(g, q), i
    assert any(not torch.equal(g, q) for g, q in zip(got, packs0))
    ex.swap_weights(data, ema)
    torch.cuda.synchronize()
    assert torch.equal(big, big0)
    for i, (g, q) in enumerate(zip(_snapshot(ex), packs0)):
        assert torch.equal(g, q), i


# ---------------------------------------------------------------- whole step
def _models(seed=0):
    from can_distributed_pytorch_amd.models import CANNet
    torch.manual_seed(seed)
    ref = CANNet(backend="torch")
    # He init so the signal survives 16 ReLU layers in a short test
    for m in ref.modules():
        if isinstance(m, torch.nn.Conv2d):
            fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
            torch.nn.init.normal_(m.weight, std=(2.0 / fan_in) ** 0.5)
            if m.bias is not None:
                torch.nn.init.uniform_(m.bias, -0.05, 0.05)
    nat = copy.deepcopy(ref)
    nat.exec_backend = "hip"
    return nat.cuda()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["sgd", "adamw"])
def test_native_stepper_ema_whole_step(name, dtype):
    """Three NativeStepper steps with EMA: parameters and moments are bitwise those of an EMA-off stepper on a deep
    copy (the same opt_step without the EMA arena), e is within the bound of the float64 recurrence over that stepper's
    weights, and the update count is 3."""
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    nat = _models(2)
    off_model = copy.deepcopy(nat)
    kw = dict(dtype=dtype, lr=1e-4 if name == "adamw" else 1e-7, graph=False, optimizer=name,
              weight_decay=1e-2 if name == "adamw" else 0.0)
    st = NativeStepper("cuda", model=nat, ema_decay=DECAY, **kw)
    off = NativeStepper("cuda", model=off_model, **kw)
    assert off.ema is None and off.ema_t is None and st.ema.data_ptr() != st.arena.data.data_ptr()
    assert torch.equal(st.ema, st.arena.data)
    x = torch.randn(2, 3, 64, 64, device="cuda")
    gt = torch.rand(2, 1, 8, 8, device="cuda")
    e0, rec = st.ema.clone(), []
    for _ in range(3):
        st.step(x, gt)
        off.step(x, gt)
        rec.append(off.arena.data.clone())
    torch.cuda.synchronize()
    assert not st.nonfinite() and not st.skipped_last() and int(st.ema_t) == 3
    assert torch.equal(st.arena.data, off.arena.data) and torch.equal(st.mom, off.mom)
    assert not torch.equal(rec[0], e0)
    if name == "adamw":
        assert torch.equal(st.mom2, off.mom2) and int(st.opt_t) == int(off.opt_t) == 3
    ref, A = _recurrence(e0, rec, DECAY, True, 0, torch.float64)
    live = A > 0
    err = ((st.ema.double() - ref).abs()[live] / A[live]).max()
    print(f"whole step {name} {dtype}: max|e-e64|/A {float(err):.3e} (bound {3 * 2.0 ** -22:.3e})")
    assert float(err) <= 3 * 2.0 ** -22
    assert bool((st.ema[~live] == 0).all()) and not torch.equal(st.ema, st.arena.data)
    es = st.ema_state()
    assert es["steps"] == 3 and list(es["ema"]) == [n for n, _ in st.model.named_parameters()]
    for (n, p), (o, c) in zip(st.model.named_parameters(), st.arena.offsets):
        assert torch.equal(es["ema"][n], st.ema[o:o + c].view_as(p)), n


# ---------------------------------------------------------------- captured replay
def _pair(dtype, steps, **kw):
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    nat_a = _models(7)
    nat_b = copy.deepcopy(nat_a)
    x = torch.randn(2, 3, 128, 192, device="cuda")
    gt = torch.rand(2, 1, 16, 24, device="cuda")
    a = NativeStepper("cuda", dtype=dtype, lr=1e-7, graph=False, model=nat_a, ema_decay=DECAY, **kw)
    b = NativeStepper("cuda", dtype=dtype, lr=1e-7, graph=True, model=nat_b, ema_decay=DECAY, **kw)
    applied = 0
    for _ in range(steps):
        a.step(x, gt)
        b.step(x, gt)
        applied += 0 if a.skipped_last() else 1
    torch.cuda.synchronize()
    return a, b, applied, (x, gt)


def _same_state(a, b):
    assert torch.equal(a.arena.data, b.arena.data) and torch.equal(a.mom, b.mom)
    assert torch.equal(a.ema, b.ema), float((a.ema - b.ema).abs().max())
    assert int(a.ema_t) == int(b.ema_t)


def test_captured_ema_replays_the_eager_step_bitwise():
    """Five steps with warm-up (d_n differs every step and is read from the device count)."""
    a, b, applied, _ = _pair("bf16", 5)
    assert b.graph_captures == 1 and applied == 5
    _same_state(a, b)
    assert int(a.ema_t) == 5 and not torch.equal(a.ema, a.arena.data)


def test_captured_ema_fp16_overflow_steps_do_not_count():
    """fp16 from a loss scale of 2^40: the first steps overflow and are skipped (flags[2]); the EMA and its count
    advance only on applied steps, eager and captured alike."""
    a, b, applied, (x, gt) = _pair("fp16", 4, init_scale=2.0 ** 40)
    assert applied == 0 and int(a.ema_t) == int(b.ema_t) == 0
    assert torch.equal(a.ema, a.arena.data) and torch.equal(b.ema, b.arena.data)
    _same_state(a, b)
    for _ in range(36):
        a.step(x, gt)
        b.step(x, gt)
        applied += 0 if a.skipped_last() else 1
    torch.cuda.synchronize()
    assert 0 < applied < 40, (applied, a.loss_scale())
    assert int(a.ema_t) == int(b.ema_t) == applied
    _same_state(a, b)


# ---------------------------------------------------------------- evaluation, accumulation, resume
def test_evaluation_under_ema_weights(tmp_path):
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    from can_distributed_pytorch_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    st = NativeStepper("cuda", lr=1e-7, graph=False, model=_models(3), ema_decay=DECAY, accum_steps=2)
    x = torch.randn(2, 3, 64, 64, device="cuda")
    gt = torch.rand(2, 1, 8, 8, device="cuda")
    for i in range(4):
        out = st.step(x, gt)
        assert (out is None) == (i % 2 == 0)
    torch.cuda.synchronize()
    assert int(st.ema_t) == 2                                    # once per window, not per micro-step
    st.model.eval()
    with torch.no_grad():
        y_raw = st.model(x).clone()
    raw, avg = st.arena.data.clone(), st.ema.clone()
    path = str(tmp_path / "epoch_0.pth")
    with st.ema_weights():
        assert torch.equal(st.arena.data, avg) and torch.equal(st.ema, raw)
        with torch.no_grad():
            y_avg = st.model(x).clone()
        sd = st.model.state_dict()
        for (n, p), (o, c) in zip(st.model.named_parameters(), st.arena.offsets):
            assert torch.equal(sd[n], avg[o:o + c].view_as(p)), n
        save_checkpoint(st.model, path)
        assert all(torch.equal(v, sd[k]) for k, v in st.ema_state()["ema"].items())
        with pytest.raises(RuntimeError, match="ema_weights"):
            st.step(x, gt)
    torch.cuda.synchronize()
    assert torch.equal(st.arena.data, raw) and torch.equal(st.ema, avg)
    with torch.no_grad():
        assert torch.equal(st.model(x), y_raw)
    assert not torch.equal(y_avg, y_raw)
    # a second native model loaded from the checkpoint saved inside the context computes the same output
    other = _models(4)
    load_checkpoint(other, path)
    other.eval()
    with torch.no_grad():
        assert torch.equal(other(x), y_avg)
    # an open window refuses
    st.model.train()
    st.step(x, gt)
    with pytest.raises(RuntimeError, match="window"):
        with st.ema_weights():
            pass
    st.flush()
    torch.cuda.synchronize()
    assert int(st.ema_t) == 3
    with st.ema_weights():
        pass
    off = NativeStepper("cuda", lr=1e-7, graph=False, model=_models(3))
    with pytest.raises(RuntimeError, match="off"):
        with off.ema_weights():
            pass
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="ema_decay"):
            NativeStepper("cuda", graph=False, model=_models(3), ema_decay=bad)


def test_ema_resume_is_bitwise(tmp_path):
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    from can_distributed_pytorch_amd.utils.checkpoint import save_train_state, load_train_state
    x = torch.randn(2, 3, 64, 64, device="cuda")
    gt = torch.rand(2, 1, 8, 8, device="cuda")
    kw = dict(lr=1e-7, graph=False, ema_decay=DECAY)
    a = NativeStepper("cuda", model=_models(5), **kw)
    for _ in range(3):
        a.step(x, gt)
    b = NativeStepper("cuda", model=_models(5), **kw)
    for _ in range(2):
        b.step(x, gt)
    path = str(tmp_path / "last_state.pth")
    es = b.ema_state()
    save_train_state(path, b.model, b.mom, 0, 1.0, stepper_state=b.resume_state(), optimizer_name=b.optimizer,
                     ema=es["ema"], ema_steps=es["steps"], ema_decay=DECAY)
    c = NativeStepper("cuda", model=_models(6), **kw)
    rs = load_train_state(path, c.model, c.mom, optimizer_name=c.optimizer, restore_rng=False)
    assert rs["ema_steps"] == 2 and rs["ema_decay"] == DECAY and rs["stepper"]["ema_steps"] == 2
    c.load_resume_state(rs["stepper"])
    assert c.load_ema_state(rs["ema"], rs["ema_steps"])
    assert int(c.ema_t) == 2 and torch.equal(c.ema, b.ema)
    c.step(x, gt)
    torch.cuda.synchronize()
    assert torch.equal(c.arena.data, a.arena.data) and torch.equal(c.ema, a.ema) and int(c.ema_t) == int(a.ema_t) == 3
    # a state without an average: the average restarts from the loaded weights at n = 0
    assert not c.load_ema_state(None)
    assert int(c.ema_t) == 0 and torch.equal(c.ema, c.arena.data)


# ---------------------------------------------------------------- the operator
def test_ema_op_opcheck_and_values():
    import can_distributed_pytorch_amd.ops.library  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    C = _C()
    n = 4099
    gen = torch.Generator(device="cuda").manual_seed(3)
    e, p = (torch.randn(n, device="cuda", generator=gen) for _ in range(2))
    torch.library.opcheck(torch.ops.cannet.ema_.default, (e.clone(), p, DECAY, True, 5),
                          test_utils=("test_schema", "test_faketensor"))
    for warmup, step in ((True, 5), (False, 1), (True, 2000)):
        e1, e2 = e.clone(), e.clone()
        torch.ops.cannet.ema_(e1, p, DECAY, warmup, step)
        C.ema(e2.data_ptr(), p.data_ptr(), n, DECAY, int(warmup), step, 0, 0, _stream())
        torch.cuda.synchronize()
        assert torch.equal(e1, e2) and not torch.equal(e1, e)
    # one float off 16-byte alignment: the same kernel's element-wise path, the same values
    buf = [torch.zeros(n + 1, device="cuda") for _ in range(2)]
    q = [b[1:] for b in buf]
    q[0].copy_(e)
    q[1].copy_(p)
    torch.ops.cannet.ema_(q[0], q[1], DECAY, True, 2000)
    assert torch.equal(q[0], e1)
    with FakeTensorMode():
        fe, fp = torch.empty(7, 3, device="cuda"), torch.empty(7, 3, device="cuda")
        assert torch.ops.cannet.ema_(fe, fp, DECAY) is None and fe.shape == (7, 3)
    with pytest.raises(ValueError):
        torch.ops.cannet.ema_(e.clone(), p, 1.0)
    with pytest.raises(ValueError):
        torch.ops.cannet.ema_(e.clone(), p[:-1], DECAY)
