"""The native optimizers beyond SGD-momentum (elementwise.hip: adam_kernel, pack_multi_kernel<DT, OPT_SGD_WD / OPT_ADAM>,
opt_tick_kernel) on the GPU: values against torch.optim in float64, the fused step against the two-launch step bit for
bit, the skip flags, the whole NativeStepper step, captured replay, resume and the custom operator.

Numerics measured on an MI355X are recorded in profiles/r7/optimizer_numerics.txt."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
VARIANTS = {"plain": (0.0, False), "coupled": (5e-4, False), "decoupled": (1e-2, True)}
SIZES = (1, 3, 4, 5, 4099, 2 ** 20 + 1)


def _C():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _torch_adam(p0, grads, wd, decoupled, dtype, m0=None, v0=None, step0=0):
    """torch.optim.Adam / AdamW (foreach=False) over the recorded gradients in ``dtype``; returns p, m, v."""
    q = p0.to(dtype).clone().requires_grad_(True)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([q], lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, foreach=False)
    if step0:
        opt.state[q] = {"step": torch.tensor(float(step0)), "exp_avg": m0.to(dtype).clone(),
                        "exp_avg_sq": v0.to(dtype).clone()}
    for g in grads:
        q.grad = g.to(dtype)
        opt.step()
    s = opt.state[q]
    assert int(s["step"]) == step0 + len(grads)
    return q.detach(), s["exp_avg"], s["exp_avg_sq"]


def _native_adam(p0, grads, wd, decoupled, misalign, m0=None, v0=None, step0=0):
    """C.adam over buffers whose base is 16-B aligned (misalign 0) or one float past it."""
    C = _C()
    n = p0.numel()
    bufs = [torch.zeros(n + 8, device="cuda") for _ in range(4)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    p, m, v, g = (b[misalign:misalign + n] for b in bufs)
    p.copy_(p0)
    if step0:
        m.copy_(m0)
        v.copy_(v0)
    t = torch.full((1,), step0, dtype=torch.int32, device="cuda")
    for gi in grads:
        g.copy_(gi)
        C.adam(p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), n, LR, BETAS[0], BETAS[1], EPS, wd,
               int(decoupled), 1.0, 0, t.data_ptr(), 0, 0, _stream())
    torch.cuda.synchronize()
    assert int(t) == step0 + len(grads)
    for b in bufs:          # nothing written outside the span
        assert float(b[:misalign].abs().sum()) == 0 and float(b[misalign + n:].abs().sum()) == 0
    return p.clone(), m.clone(), v.clone()


def _errors(got, ref64, A):
    """The three metrics.  Elements whose running max of |g| is 0 have no scale for m and v (coupled weight decay
    still moves them by wd * p): they count in the p metric only."""
    p, m, v = got
    p64, m64, v64 = ref64
    live = A > 0
    if not bool(live.any()):
        return float((p.double() - p64).abs().max()) / LR, 0.0, 0.0
    Al = A[live]
    return (float((p.double() - p64).abs().max()) / LR, float(((m.double() - m64).abs()[live] / Al).max()),
            float(((v.double() - v64).abs()[live] / (Al * Al)).max()))


def _adam_case(variant, T, step0=0, sizes=SIZES):
    wd, decoupled = VARIANTS[variant]
    gen = torch.Generator(device="cuda").manual_seed(1234 + T + step0)
    rows = []
    for n in sizes:
        scale = 10.0 ** torch.randint(-4, 3, (n,), device="cuda", generator=gen).float()
        grads = [torch.randn(n, device="cuda", generator=gen) * scale for _ in range(T)]
        p0 = torch.randn(n, device="cuda", generator=gen)
        m0 = v0 = None
        A = torch.stack([g.abs() for g in grads]).max(0).values.double()
        if step0:
            m0 = 0.3 * scale * torch.randn(n, device="cuda", generator=gen)
            v0 = (scale * torch.rand(n, device="cuda", generator=gen)) ** 2
            A = torch.maximum(A, torch.maximum(m0.abs(), v0.sqrt()).double())
        ref64 = _torch_adam(p0, grads, wd, decoupled, torch.float64, m0, v0, step0)
        e_t = _errors(_torch_adam(p0, grads, wd, decoupled, torch.float32, m0, v0, step0), ref64, A)
        for mis in (0, 1):
            got = _native_adam(p0, grads, wd, decoupled, mis, m0, v0, step0)
            e = _errors(got, ref64, A)
            rows.append((n, mis, e, e_t))
            if T == 1 and wd == 0 and not step0:
                # closed form of the first step: m / (sqrt(v) + eps) = sign(g) up to eps / |g|
                big = grads[0].abs() >= 1e-4
                dev = ((got[0] - p0) + LR * torch.sign(grads[0]))[big].abs()
                assert dev.numel() == 0 or float(dev.max()) <= 1e-3 * LR, (n, mis, float(dev.max()))
    for n, mis, e, e_t in rows:
        print(f"adam {variant:9s} T={T:2d} t0={step0:4d} n={n:7d} mis={mis} "
              f"p {e[0]:.3e} (torch {e_t[0]:.3e})  m {e[1]:.3e} ({e_t[1]:.3e})  v {e[2]:.3e} ({e_t[2]:.3e})")
    # the yardstick: torch.optim in fp32 on the same inputs against the same float64 run, size by size
    for n, mis, e, e_t in rows:
        for k, name in enumerate("pmv"):
            assert e[k] <= 4 * e_t[k], (variant, T, n, mis, name, e[k], e_t[k])
    return rows


@pytest.mark.parametrize("T", [1, 25])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_adam_kernel_values(variant, T):
    """C.adam against torch.optim.Adam / AdamW in float64 on the same inputs: max|p - p64| / lr, max|m - m64| / A and
    max|v - v64| / A^2 (A = running max of |g| per element) are each at most 4x what torch.optim in fp32 shows against
    the same float64 run on the same inputs, for every size on its own; T = 1, wd = 0: the closed form p1 = p0 - lr * sign(g)."""
    _adam_case(variant, T)


def test_adam_kernel_bias_correction_at_step_1000():
    """The device step count preset to 1000 (torch: state['step'] = 1000): pins the bias-correction path."""
    _adam_case("plain", 1, step0=1000, sizes=(5, 4099))
    _adam_case("decoupled", 3, step0=1000, sizes=(4099,))


def test_adam_kernel_skip_flags():
    C = _C()
    n = 4099
    p, m, v, g = (torch.randn(n, device="cuda") for _ in range(4))
    v.abs_()
    t = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    before = [x.clone() for x in (p, m, v)]
    for idx in (0, 2):
        flags = torch.zeros(4, device="cuda")
        flags[idx] = 1.0
        C.adam(p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), n, LR, 0.9, 0.999, EPS, 0.0, 0, 1.0, 0,
               t.data_ptr(), flags.data_ptr(), 0, _stream())
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((p, m, v), before)) and int(t) == 7
        assert float(flags[3]) == (1.0 if idx == 0 else 0.0)
    # clean flags: applied, the count advances, and lr comes from the device scalar when one is given
    flags = torch.zeros(4, device="cuda")
    lr_dev = torch.tensor([LR], device="cuda")
    p2, m2, v2 = (x.clone() for x in before)
    t2 = t.clone()
    C.adam(p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), n, 123.0, 0.9, 0.999, EPS, 0.0, 0, 1.0, 0,
           t.data_ptr(), flags.data_ptr(), lr_dev.data_ptr(), _stream())
    C.adam(p2.data_ptr(), m2.data_ptr(), v2.data_ptr(), g.data_ptr(), n, LR, 0.9, 0.999, EPS, 0.0, 0, 1.0, 0,
           t2.data_ptr(), 0, 0, _stream())
    torch.cuda.synchronize()
    assert int(t) == int(t2) == 8 and not torch.equal(p, before[0])
    assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2)


# ---------------------------------------------------------------- fused == two-launch
def _arena(layout):
    """A full CANNet whose parameters are views of a flat master arena, with gradient / first / second-moment arenas
    carved from one buffer.  layout: 'aligned' (all 16-B aligned), 'offset1' (every arena one float past alignment:
    element-wise paths, offsets between the arenas still whole float4s) or 'g_mod4_1' / 'b_mod4_1' / 'v_mod4_1'
    (masters aligned, the gradient / first-moment / second-moment arena 1 (mod 4) floats from them: the v4 guard must
    send the step down the element-wise path).  The values do not depend on the layout."""
    from can_distributed_pytorch_amd.models import CANNet
    torch.manual_seed(9)
    model = CANNet().cuda()
    ps = list(model.parameters())
    k = sum(p.numel() for p in ps)
    pad = -(-k // 4) * 4 + 8
    big = torch.zeros(4 * pad + 8, device="cuda")
    assert big.data_ptr() % 16 == 0
    o = 1 if layout == "offset1" else 0
    starts = [o, pad + o + (layout == "g_mod4_1"), 2 * pad + o + (layout == "b_mod4_1"),
              3 * pad + o + (layout == "v_mod4_1")]
    data, grad, mom, mom2 = (big[s:s + k] for s in starts)
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


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("layout", ["aligned", "offset1", "v_mod4_1"])
def test_fused_adam_pack_matches_two_launch_step(layout, dtype):
    """executor.opt_step (Adam + the 16-bit packs, one launch + the step-count tick) == C.adam over the parameter span
    followed by pack_multi, bit for bit: masters, both moments, the step count, every fwd / dgrad pack and the
    interleaved context packs.  Then the skip flags: flags[0] leaves everything untouched and latches flags[3],
    flags[2] leaves everything, the step count included, untouched."""
    from can_distributed_pytorch_amd.engine.native import ACT_DTYPES
    from can_distributed_pytorch_amd.ops.executor import CANNetExecutor
    C = _C()
    model, big, data, grad, mom, mom2 = _arena(layout)
    ex = CANNetExecutor(model, dtype=ACT_DTYPES[dtype])
    ex.refresh_packs(force=True)
    flags = torch.zeros(4, device="cuda")
    lr_dev = torch.tensor([3e-3], device="cuda")
    hp = dict(optimizer="adamw", weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8)
    big0 = big.clone()
    t_ref = torch.full((1,), 11, dtype=torch.int32, device="cuda")
    C.adam(data.data_ptr(), mom.data_ptr(), mom2.data_ptr(), grad.data_ptr(), data.numel(), 1.0, 0.9, 0.999, 1e-8,
           1e-2, 1, 0.5, 0, t_ref.data_ptr(), flags.data_ptr(), lr_dev.data_ptr(), _stream())
    ex.refresh_packs(force=True)
    torch.cuda.synchronize()
    ref_big, ref_packs = big.clone(), _snapshot(ex)
    assert not torch.equal(ref_big, big0)
    with torch.no_grad():
        big.copy_(big0)
    ex.refresh_packs(force=True)
    t = torch.full((1,), 11, dtype=torch.int32, device="cuda")
    ex.opt_step(data, grad, mom, 1.0, 0.5, mom2=mom2, step=t, flags=flags, lr_dev=lr_dev, **hp)
    torch.cuda.synchronize()
    assert torch.equal(big, ref_big), float((big - ref_big).abs().max())
    assert int(t) == int(t_ref) == 12
    for i, (g, r) in enumerate(zip(_snapshot(ex), ref_packs)):
        assert torch.equal(g, r), i
    # skip semantics
    before_big, before_packs = big.clone(), _snapshot(ex)
    for idx in (0, 2):
        flags.zero_()
        flags[idx] = 1.0
        ex.opt_step(data, grad, mom, 1.0, 0.5, mom2=mom2, step=t, flags=flags, lr_dev=lr_dev, **hp)
        torch.cuda.synchronize()
        assert torch.equal(big, before_big) and int(t) == 12
        assert all(torch.equal(a, b) for a, b in zip(_snapshot(ex), before_packs))
        assert float(flags[3]) == (1.0 if idx == 0 else 0.0)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("layout", ["aligned", "offset1", "g_mod4_1", "b_mod4_1"])
def test_fused_sgd_weight_decay_pack(layout, dtype):
    """executor.opt_step('sgd', weight_decay=5e-4) against fp32 torch ops in the kernel's order (g' = gscale*g + wd*p;
    buf = momentum*buf + g'; p -= lr*buf).  The kernel fuses the multiply-adds, torch rounds each product, so the
    masters agree to allclose(rtol=2e-7) (one ulp of buf is 1.2e-7 relative and enters p scaled by lr = 3e-3; the
    momentum itself can lose a digit where momentum*buf and g' cancel: rtol 1e-5 of max(|momentum*buf|, |g'|)); the
    packs are exactly the re-pack of the fused masters."""
    from can_distributed_pytorch_amd.engine.native import ACT_DTYPES
    from can_distributed_pytorch_amd.ops.executor import CANNetExecutor
    model, big, data, grad, mom, _ = _arena(layout)
    ex = CANNetExecutor(model, dtype=ACT_DTYPES[dtype])
    ex.refresh_packs(force=True)
    flags = torch.zeros(4, device="cuda")
    lr, wd, mu, gs = 3e-3, 5e-4, 0.95, 0.5
    lr_dev = torch.tensor([lr], device="cuda")
    d0, m0 = data.clone(), mom.clone()
    g1 = grad * gs + wd * d0
    b_ref = mu * m0 + g1
    p_ref = d0 - lr * b_ref
    ex.opt_step(data, grad, mom, 1.0, gs, optimizer="sgd", momentum=mu, weight_decay=wd, flags=flags, lr_dev=lr_dev)
    torch.cuda.synchronize()
    assert torch.allclose(data, p_ref, rtol=2e-7), float((data - p_ref).abs().max())
    assert bool(((mom - b_ref).abs() <= 1e-5 * torch.maximum((mu * m0).abs(), g1.abs())).all())
    # wd really entered: the wd = 0 result differs
    assert not torch.allclose(data, d0 - lr * (mu * m0 + grad * gs), rtol=2e-7)
    got = _snapshot(ex)
    ex.refresh_packs(force=True)
    torch.cuda.synchronize()
    for i, (g, r) in enumerate(zip(got, _snapshot(ex))):
        assert torch.equal(g, r), i
    before = big.clone()
    flags[0] = 1.0
    ex.opt_step(data, grad, mom, 1.0, gs, optimizer="sgd", momentum=mu, weight_decay=wd, flags=flags, lr_dev=lr_dev)
    torch.cuda.synchronize()
    assert torch.equal(big, before) and float(flags[3]) == 1.0


@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_fused_sgd_state_arena_off_float4_alignment(wd):
    """The v4 guard on the SGD kinds (wd = 0: the instantiation of before): a gradient or momentum arena 1 (mod 4)
    floats from 16-byte-aligned masters takes the element-wise path and gives the aligned layout's masters, momentum
    and bf16 packs bit for bit (both paths run the same explicit multiply / fma per element)."""
    from can_distributed_pytorch_amd.engine.native import ACT_DTYPES
    from can_distributed_pytorch_amd.ops.executor import CANNetExecutor
    out = {}
    for layout in ("aligned", "g_mod4_1", "b_mod4_1"):
        model, big, data, grad, mom, _ = _arena(layout)
        ex = CANNetExecutor(model, dtype=ACT_DTYPES["bf16"])
        ex.refresh_packs(force=True)
        d0 = data.clone()
        ex.opt_step(data, grad, mom, 3e-3, 0.5, optimizer="sgd", momentum=0.95, weight_decay=wd)
        torch.cuda.synchronize()
        assert not torch.equal(data, d0)
        out[layout] = (data.clone(), mom.clone(), _snapshot(ex))
        del model, big, ex
    ref = out["aligned"]
    for layout in ("g_mod4_1", "b_mod4_1"):
        got = out[layout]
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), layout
        for i, (g, r) in enumerate(zip(got[2], ref[2])):
            assert torch.equal(g, r), (layout, i)


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


@pytest.mark.parametrize("name,wd", [("adam", 0.0), ("adamw", 1e-2)])
def test_native_stepper_adam_matches_torch_optim(name, wd):
    """Three NativeStepper steps == torch.optim.Adam / AdamW on a deep copy fed the stepper's own arena gradients."""
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    nat = _models(2)
    ref = copy.deepcopy(nat)
    lr = 1e-4
    cls = torch.optim.AdamW if name == "adamw" else torch.optim.Adam
    opt = cls(ref.parameters(), lr=lr, weight_decay=wd, foreach=False)
    st = NativeStepper("cuda", lr=lr, graph=False, model=nat, optimizer=name, weight_decay=wd)
    x = torch.randn(2, 3, 64, 64, device="cuda")
    gt = torch.rand(2, 1, 8, 8, device="cuda")
    for _ in range(3):
        st.step(x, gt)
        for q, g in zip(ref.parameters(), st.grads):
            q.grad = g.detach().clone()
        opt.step()
    torch.cuda.synchronize()
    assert not st.nonfinite() and int(st.opt_t) == 3
    for (n, a), b in zip(ref.named_parameters(), nat.parameters()):
        assert torch.allclose(b, a, rtol=1e-5, atol=1e-2 * lr), (n, float((a - b).abs().max()))


def _pair(dtype, steps, **kw):
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    nat_a = _models(7)
    nat_b = copy.deepcopy(nat_a)
    x = torch.randn(2, 3, 128, 192, device="cuda")
    gt = torch.rand(2, 1, 16, 24, device="cuda")
    a = NativeStepper("cuda", dtype=dtype, lr=1e-4, graph=False, model=nat_a, optimizer="adam", **kw)
    b = NativeStepper("cuda", dtype=dtype, lr=1e-4, graph=True, model=nat_b, optimizer="adam", **kw)
    applied = 0
    for _ in range(steps):
        a.step(x, gt)
        b.step(x, gt)
        applied += 0 if a.skipped_last() else 1
    torch.cuda.synchronize()
    return a, b, applied


def _same_state(a, b):
    for pa, pb in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(pa, pb), float((pa - pb).abs().max())
    assert torch.equal(a.mom, b.mom) and torch.equal(a.mom2, b.mom2)


def test_captured_adam_replays_the_eager_step_bitwise():
    a, b, applied = _pair("bf16", 4)
    assert b.graph_captures == 1 and applied == 4
    _same_state(a, b)
    assert int(a.opt_t) == int(b.opt_t) == 4
    assert float(a.mom2.abs().max()) > 0


def test_captured_adam_fp16_overflow_steps_do_not_count():
    """fp16 from a loss scale of 2^40: the first steps overflow and are skipped (flags[2]); the device step count
    advances only on applied steps, eager and captured alike.  The first four steps are all skipped; the run goes on
    until the scale has backed off so that applied steps are covered too."""
    a, b, applied = _pair("fp16", 4, init_scale=2.0 ** 40)
    assert applied == 0 and int(a.opt_t) == int(b.opt_t) == 0
    assert float(a.mom.abs().max()) == 0 and float(a.mom2.abs().max()) == 0
    _same_state(a, b)
    x = torch.randn(2, 3, 128, 192, device="cuda")
    gt = torch.rand(2, 1, 16, 24, device="cuda")
    for _ in range(36):
        a.step(x, gt)
        b.step(x, gt)
        applied += 0 if a.skipped_last() else 1
    torch.cuda.synchronize()
    assert 0 < applied < 40, (applied, a.loss_scale())
    assert int(a.opt_t) == int(b.opt_t) == applied
    _same_state(a, b)


def test_adam_resume_is_bitwise(tmp_path):
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    from can_distributed_pytorch_amd.utils.checkpoint import save_train_state, load_train_state
    x = torch.randn(2, 3, 64, 64, device="cuda")
    gt = torch.rand(2, 1, 8, 8, device="cuda")
    kw = dict(lr=1e-4, graph=False, optimizer="adam", weight_decay=1e-3)
    a = NativeStepper("cuda", model=_models(5), **kw)
    for _ in range(4):
        a.step(x, gt)
    b = NativeStepper("cuda", model=_models(5), **kw)
    for _ in range(2):
        b.step(x, gt)
    path = str(tmp_path / "last_state.pth")
    save_train_state(path, b.model, b.mom, 0, 1.0, stepper_state=b.resume_state(), momentum2=b.mom2,
                     optimizer_name=b.optimizer)
    c = NativeStepper("cuda", model=_models(6), **kw)
    rs = load_train_state(path, c.model, c.mom, momentum2=c.mom2, optimizer_name=c.optimizer, restore_rng=False)
    c.load_resume_state(rs["stepper"])
    assert int(c.opt_t) == 2
    for _ in range(2):
        c.step(x, gt)
    torch.cuda.synchronize()
    for pa, pc in zip(a.model.parameters(), c.model.parameters()):
        assert torch.equal(pa, pc), float((pa - pc).abs().max())
    assert int(c.opt_t) == int(a.opt_t) == 4
    s = NativeStepper("cuda", model=_models(6), lr=1e-4, graph=False)
    with pytest.raises(ValueError, match="adam"):
        s.load_resume_state(rs["stepper"])


def test_adam_op_opcheck_and_values():
    import can_distributed_pytorch_amd.ops.library  # noqa: F401
    C = _C()
    n = 4099
    gen = torch.Generator(device="cuda").manual_seed(3)
    p, m, g = (torch.randn(n, device="cuda", generator=gen) for _ in range(3))
    v = torch.rand(n, device="cuda", generator=gen)
    args = (5, 1e-3, 0.9, 0.999, 1e-8, 1e-2, True, 0.5)
    torch.library.opcheck(torch.ops.cannet.adam_.default, (p.clone(), m.clone(), v.clone(), g) + args,
                          test_utils=("test_schema", "test_faketensor"))
    # values: C.adam's bit for bit, the 3-element tail included
    p1, m1, v1 = p.clone(), m.clone(), v.clone()
    torch.ops.cannet.adam_(p1, m1, v1, g, *args)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    C.adam(p2.data_ptr(), m2.data_ptr(), v2.data_ptr(), g.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 0.5, 5, 0, 0,
           0, _stream())
    torch.cuda.synchronize()
    for x1, x2 in ((p1, p2), (m1, m2), (v1, v2)):
        assert torch.equal(x1, x2)
    assert not torch.equal(p1, p)
    # unaligned tensors take the ATen fallback and agree with the kernel closely
    buf = [torch.zeros(n + 1, device="cuda") for _ in range(4)]
    q = [b[1:] for b in buf]
    for dst, src in zip(q, (p, m, v, g)):
        dst.copy_(src)
    torch.ops.cannet.adam_(q[0], q[1], q[2], q[3], *args)
    assert torch.allclose(q[0], p2, rtol=1e-5, atol=1e-8) and torch.allclose(q[2], v2, rtol=1e-5, atol=1e-12)


def test_loss_decreases_native_adam():
    """A few native Adam steps on one batch reduce the loss."""
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch
    from can_distributed_pytorch_amd.models import CANNet
    torch.manual_seed(5)
    m = CANNet().cuda()
    img, gt = make_synthetic_batch(2, 128, 128, seed=5, device="cuda")
    st = NativeStepper("cuda", lr=1e-5, graph=False, model=m, optimizer="adam")
    losses = [float(st.step(img, gt)) for _ in range(8)]
    assert losses[-1] < losses[0], losses
