"""GPU tests of the step runtime: owned context GEMMs, device-side flags, device lr, headline-shape numerics."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SCALES = (1, 2, 3, 6)
CELL_OFF = {1: 0, 2: 1, 3: 5, 6: 14}


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.mark.parametrize("n", [1, 3, 8, 15])
def test_ctx_gemm_all_modes_vs_fp32(n):
    """conv{S}_1 forward / data-gradient / weight-gradient of all four scales (one launch each) vs torch fp32.
    Batch 15 runs the tiled kernel, the others the matrix-core one (bit for bit: tests/test_gpu_ctx_gemm_exact.py)."""
    from can_distributed_pytorch_amd.ops import _ext
    C = _ext.require()
    c = 512
    torch.manual_seed(n)
    ave = torch.randn(n, 50, c, device="cuda")
    dA = torch.randn(n, 50, c, device="cuda")
    ws = [torch.randn(c, c, device="cuda") * 0.05 for _ in SCALES]
    st = torch.cuda.current_stream().cuda_stream
    table = torch.full_like(ave, float("nan"))
    C.ctx_gemm(0, ave.data_ptr(), 0, [w.data_ptr() for w in ws], table.data_ptr(), [], n, c, 0.0, 1.0, 0, st)
    dave = torch.full_like(ave, float("nan"))
    C.ctx_gemm(1, dA.data_ptr(), 0, [w.data_ptr() for w in ws], dave.data_ptr(), [], n, c, 0.0, 1.0, 0, st)
    gws = [torch.full((c, c), 3.0, device="cuda") for _ in SCALES]
    dsc = torch.tensor([0.5], device="cuda")
    C.ctx_gemm(2, dA.data_ptr(), ave.data_ptr(), [], 0, [g.data_ptr() for g in gws], n, c, 1.0, 2.0,
               dsc.data_ptr(), st)
    torch.cuda.synchronize()
    for w, sc, g in zip(ws, SCALES, gws):
        o, k = CELL_OFF[sc], sc * sc
        a_, d_ = ave[:, o:o + k].reshape(-1, c).double(), dA[:, o:o + k].reshape(-1, c).double()
        assert torch.allclose(table[:, o:o + k].reshape(-1, c).double(), a_ @ w.double().t(), rtol=1e-4, atol=1e-4)
        assert torch.allclose(dave[:, o:o + k].reshape(-1, c).double(), d_ @ w.double(), rtol=1e-4, atol=1e-4)
        # beta = 1 accumulates, scale * dscale = 1.0 multiplies the fresh product
        assert torch.allclose(g.double(), 3.0 + d_.t() @ a_, rtol=1e-4, atol=1e-3)


def _stepper(seed=0, **kw):
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    from can_distributed_pytorch_amd.models import CANNet
    torch.manual_seed(seed)
    return NativeStepper("cuda", model=CANNet().cuda(), **kw)


def test_nonfinite_flag_is_sticky_and_skips_the_update():
    """A NaN loss on a step the host does not read (not a multiple of the logging cadence) still latches the
    device flag, and that step's update is skipped (sticky non-finite flag)."""
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch
    st = _stepper(1, lr=1e-6, graph=False)
    img, gt = make_synthetic_batch(1, 64, 64, seed=1, device="cuda")
    bad = gt.clone()
    bad[0, 0, 1, 1] = float("nan")
    st.step(img, gt)
    st.step(img, gt)
    before = st.arena.data.clone()
    st.step(img, bad)                      # step 3: NaN
    torch.cuda.synchronize()
    assert torch.equal(st.arena.data, before)          # update skipped
    st.step(img, gt)
    st.step(img, gt)
    assert st.nonfinite()                  # still latched two clean steps later
    assert bool(torch.isfinite(st.arena.data).all())
    st.reset_nonfinite()
    st.step(img, gt)
    assert not st.nonfinite()


def test_graph_replay_follows_device_lr():
    """lr lives in a device scalar: changing stepper.lr between replays of one captured step takes effect
    (the lr of a captured step used to be frozen at capture time)."""
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch
    st = _stepper(2, lr=1e-6, graph=True)
    img, gt = make_synthetic_batch(1, 64, 64, seed=2, device="cuda")
    st.step(img, gt)                       # capture + first replay
    st.lr = 0.0
    before = st.arena.data.clone()
    st.step(img, gt)
    torch.cuda.synchronize()
    assert torch.equal(st.arena.data, before)          # lr 0: no movement (momentum buffer still advances)
    st.lr = 1e-6
    st.step(img, gt)
    torch.cuda.synchronize()
    assert not torch.equal(st.arena.data, before)


def test_headline_shape_gradients_vs_fp32():
    """Whole-network gradients at the benchmark's own shape (768x1024; batch 2 instead of 8 to fit the fp32
    reference) — exercises the dispatch the bench takes (128x512 tiles, fused pools, row-ring wgrad, halo
    kernels) — vs fp32 ATen, under the same rule as the small-shape test: each parameter's relative gradient
    error <= 1.5x that of PyTorch's own bf16 path (autocast, MIOpen), or < 5e-2."""
    from can_distributed_pytorch_amd.models import CANNet
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch
    torch.manual_seed(11)
    ref = CANNet(backend="torch")
    for m in ref.modules():
        if isinstance(m, torch.nn.Conv2d):
            fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
            torch.nn.init.normal_(m.weight, std=(2.0 / fan_in) ** 0.5)
            if m.bias is not None:
                torch.nn.init.uniform_(m.bias, -0.05, 0.05)
    nat = copy.deepcopy(ref)
    nat.exec_backend = "hip"
    ref, nat = ref.cuda(), nat.cuda()
    img, gt = make_synthetic_batch(2, 768, 1024, seed=11, device="cuda")
    crit = torch.nn.MSELoss(reduction="sum")
    crit(ref(img), gt).backward()
    crit(nat(img), gt).backward()
    am = copy.deepcopy(ref).to(memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ya = am(img.contiguous(memory_format=torch.channels_last)).float()
    crit(ya, gt).backward()
    bad, worst = [], 0.0
    for (name, pr), pn, pa in zip(ref.named_parameters(), nat.parameters(), am.parameters()):
        en, ea = _rel(pn.grad, pr.grad), _rel(pa.grad, pr.grad)
        worst = max(worst, en)
        if not (en <= max(1.5 * ea, 0.05)):
            bad.append((name, round(en, 4), round(ea, 4)))
    print("worst native relative gradient error", worst)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# Production-step gradient fidelity: the NativeStepper's own step (arena, bucket views, bias partials, side stream)
# ---------------------------------------------------------------------------------------------------------------------
def _native_step_capture(seed, n, h, w, perturb=None):
    """One native training step (no update) at [n,3,h,w]; records every layer's weight-gradient operands (dY, X) as
    the executor hands them to conv_wgrad, plus the head's b6 / et and the saved forward state.
    perturb: None | "swap_views" (two same-shape weight gradients written into each other's arena slot: a wrong
    bucket / slot offset) | "bias_row" (one row of one data-gradient epilogue's bias partials zeroed) |
    "pool_codes" (conv2_2's saved max-pool codes shifted by one pooled column: valid codes at the wrong pixels)."""
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch
    from can_distributed_pytorch_amd.ops import conv as C
    st = _stepper(seed, lr=1e-7, graph=False)
    ex = st.ex
    for m in st.model.modules():
        if isinstance(m, torch.nn.Conv2d):
            fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
            torch.nn.init.normal_(m.weight, std=(2.0 / fan_in) ** 0.5)
            if m.bias is not None:
                torch.nn.init.uniform_(m.bias, -0.05, 0.05)
    ex.refresh_packs(force=True)
    img, gt = make_synthetic_batch(n, h, w, seed=seed, device="cuda")
    rec = {"wgrad": [], "head": None, "sv": None}
    orig_wgrad, orig_dgb, orig_fwd, orig_head = C.conv_wgrad, C.conv_dgrad_with_bias, ex.forward_features, ex.head_train

    def wgrad(dy, x, dw, db, **kw):
        rec["wgrad"].append((dy, x, kw.get("ksize"), kw.get("dil", 1)))
        return orig_wgrad(dy, x, dw, db, **kw)

    done = [False]

    def dgb(*a, **kw):
        out, bp = orig_dgb(*a, **kw)
        if perturb == "bias_row" and bp is not None and not done[0]:
            bp[0:1].zero_()                       # stream-ordered: before the weight-gradient side stream forks
            done[0] = True
        return out, bp

    def fwd(img_, save):
        b6, sv = orig_fwd(img_, save)
        rec["sv"] = sv
        if perturb == "pool_codes":
            c = sv["pre_pool"][3]
            c.copy_(c.roll(1, dims=2))             # stream-ordered: after the forward wrote them, before the backward
        return b6, sv

    def head(b6, gt_, grads, **kw):
        loss, et, d_b6 = orig_head(b6, gt_, grads, **kw)
        rec["head"] = (b6, et, d_b6)
        return loss, et, d_b6

    grads = st.grads
    if perturb == "swap_views":
        wa, wb = ex.back[1].w_index, ex.back[2].w_index          # backend.2 / backend.4: both [512, 512, 3, 3]
        grads = list(grads)
        grads[wa], grads[wb] = grads[wb], grads[wa]
    C.conv_wgrad, C.conv_dgrad_with_bias = wgrad, dgb
    ex.forward_features, ex.head_train = fwd, head
    saved_grads = st.grads
    st.grads = grads
    try:
        st._step_body(img, gt, update=False)
        torch.cuda.synchronize()
    finally:
        C.conv_wgrad, C.conv_dgrad_with_bias = orig_wgrad, orig_dgb
        ex.forward_features, ex.head_train = orig_fwd, orig_head
        st.grads = saved_grads
    return st, img, gt, rec


def _layer_local_errors(st, img, gt, rec):
    """Every parameter's arena gradient vs an fp32 / fp64 reference computed from the SAME 16-bit operands the
    executor used for that layer (its saved input X and the dY it handed to the weight-gradient launch), so the only
    legitimate difference is summation order: weights tol 2e-3 of max|ref| (check_sum32), biases 1e-4 (fp64 sums of
    the same bf16 dY values).  Returns {param name: message} of the failures."""
    from numerics import check_sum32
    ex = st.ex
    names = [nm for nm, _ in st.model.named_parameters()]
    grads = st.arena.grad_views()               # what the reducer all-reduces and SGD applies
    sv = rec["sv"]
    ident = {}
    for s in ex.front:
        ident[sv["front_in"][s.idx].data_ptr()] = s
    for s in ex.back:
        ident[sv["back_in"][s.idx].data_ptr()] = s
    fails = {}
    seen = set()

    def check(i, got, ref, tol):
        try:
            check_sum32(got, ref, tol=tol, what=names[i])
        except AssertionError as e:
            fails[names[i]] = str(e)[:300]
        seen.add(i)

    def nchw(t):
        return t.permute(0, 3, 1, 2).float()

    conv12_dy = None
    for dy, x, ksize, dil in rec["wgrad"]:
        s = ident.get(x.data_ptr())
        if s is None or ksize != 3:
            continue      # context 1x1 weight gradients: the dW1 / dW2 stages of tests/test_gpu_context_stages.py
        if s.idx == 1 and s in ex.front:
            conv12_dy = dy
        dw = torch.nn.grad.conv2d_weight(nchw(x)[:, :s.cin], (s.cout, s.cin, 3, 3), nchw(dy), padding=dil,
                                         dilation=dil)
        check(s.w_index, grads[s.w_index], dw, 2e-3)
        check(s.b_index, grads[s.b_index], dy.double().sum((0, 1, 2)).float(), 1e-4)
    # conv1_1 (fused into conv1_2's data gradient): its dY = conv1_2's data gradient, masked by conv1_1's output,
    # rounded to 16 bits as the fused kernel feeds it to the MFMA
    f0, f1 = ex.front[0], ex.front[1]
    if conv12_dy is not None and f0.w_index not in seen:
        w12 = f1.module.weight.detach().to(conv12_dy.dtype).float()
        dx = torch.nn.grad.conv2d_input(nchw(conv12_dy).shape[:1] + (64,) + nchw(conv12_dy).shape[2:], w12,
                                        nchw(conv12_dy), padding=1)
        dx = (dx * (nchw(sv["front_in"][1]) > 0)).to(conv12_dy.dtype).float()
        x0 = nchw(sv["front_in"][0])[:, :3]
        check(f0.w_index, grads[f0.w_index], torch.nn.grad.conv2d_weight(x0, (64, 3, 3, 3), dx, padding=1), 4e-3)
        check(f0.b_index, grads[f0.b_index], dx.double().sum((0, 2, 3)).float(), 1e-3)
    # head: d(et) = 2 (et - gt); dW = sum d(et) relu(b6), db = sum d(et)
    b6, et, _ = rec["head"]
    de = 2.0 * (et.double() - gt.double()).reshape(-1, 1)
    check(ex.head_w_index, grads[ex.head_w_index].reshape(-1),
          (de * b6.double().reshape(-1, b6.shape[-1]).clamp_min(0)).sum(0).float(), 1e-4)
    check(ex.head_b_index, grads[ex.head_b_index].reshape(-1), de.sum().reshape(1).float(), 1e-4)
    return fails, seen


def test_step_gradients_layer_local():
    """The production step (NativeStepper: arena views, bucket slots, bias partials from the data-gradient
    epilogues, weight gradients on the side stream, conv1_1 fused into conv1_2's data gradient) at the bench's own
    shape: every conv / head parameter's gradient equals the reference computed from that layer's own 16-bit operands
    (weights 2e-3, biases 1e-4 of scale).  The context parameters' operands: test_step_composition_vs_teacher_forced_oracle."""
    st, img, gt, rec = _native_step_capture(21, 2, 768, 1024)
    fails, seen = _layer_local_errors(st, img, gt, rec)
    assert not fails, fails
    ex = st.ex
    want = {s.w_index for s in ex.front + ex.back} | {s.b_index for s in ex.front + ex.back} | \
        {ex.head_w_index, ex.head_b_index}
    assert want <= seen, sorted(want - seen)


def _composition_errors(st, gt, rec):
    """Teacher-forced oracle (tests/oracle.py teacher_forced_pairs): every forward layer output and every backward dY
    of the production step vs the oracle layer fed the step's own saved input / upstream dY.  Returns
    {what: (relative L2, fraction of 16-bit elements that differ, fraction routed differently)}."""
    from oracle import pair_errors, teacher_forced_pairs
    ex = st.ex
    sv = rec["sv"]
    ident = {}
    for s_, k in zip(ex.front, (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)):
        ident[sv["front_in"][s_.idx].data_ptr()] = f"frontend.{k}"
    for s_, k in zip(ex.back, (0, 2, 4, 6, 8, 10)):
        ident[sv["back_in"][s_.idx].data_ptr()] = f"backend.{k}"
    dys = {ident[x.data_ptr()]: dy for dy, x, ksize, _ in rec["wgrad"] if ksize == 3 and x.data_ptr() in ident}
    pairs = teacher_forced_pairs(st.model, sv, rec["head"], dys, gt, ex.act)
    return {what: pair_errors(a, b, ex.act) for what, a, b in pairs}


# per layer: one layer's fp32 summation order apart -> rare one-ulp flips of the 16-bit store, and rarer elements
# routed differently by a flipped ReLU mask / pool argmax (oracle.pair_errors)
COMPOSITION_REL, COMPOSITION_FLIPS, COMPOSITION_ROUTED = 2e-3, 2e-3, 2e-4


def _composition_ok(v):
    return v[0] <= COMPOSITION_REL and v[1] <= COMPOSITION_FLIPS and v[2] <= COMPOSITION_ROUTED


@pytest.mark.parametrize("n,h,w", [(1, 384, 512), (2, 768, 1024)])
def test_step_composition_vs_teacher_forced_oracle(n, h, w):
    """The production step (NativeStepper: arena, bias partials, side stream, fused conv1_1 weight gradient, fused
    pools and their codes, sign-bit masks, linearised context module, fused head) against the emulated-rounding fp32
    oracle (tests/oracle.py) layer by layer: each oracle layer is fed the step's own saved input (forward) or its own
    upstream dY (backward), and its 16-bit output must match what the step stored: relative L2 <= 2e-3, <= 0.2 % of
    the elements one ulp apart and <= 0.02 % routed differently by a flipped mask / argmax (left out of the relative
    L2: oracle.pair_errors), for all 17 forward outputs (10 frontend incl. the three fused pools, the context module's
    cat, 6 backend, et) and 16 backward dYs (head, 5 backend, context -> conv4_3, 8 frontend through the
    pool codes).  Whole-network drift is chaotic (scripts/dev/oracle_diag.py: rounding flips grow layer by layer), so
    the per-parameter gradients are pinned here layer-locally (test_step_gradients_layer_local) and by this
    composition, not end to end.  The bench's shape (768x1024) included."""
    st, img, gt, rec = _native_step_capture(23, n, h, w)
    errs = _composition_errors(st, gt, rec)
    for k, (r, f, ro) in errs.items():
        print(f"  {k:28s} rel {r:.2e}  flips {f:.5f}  routed {ro:.6f}")
    assert len(errs) == 33
    bad = {k: v for k, v in errs.items() if not _composition_ok(v)}
    assert not bad, bad


@pytest.mark.parametrize("perturb", ["swap_views", "bias_row", "pool_codes"])
def test_step_checks_catch_plumbing_bugs(perturb):
    """The whole-step checks fail on test-only plumbing bugs the per-kernel checkers cannot see: two weight gradients
    written into each other's arena slot (a wrong bucket / slot offset) and one lost bias-partial row of a
    data-gradient epilogue (layer-local gradients), conv2_2's max-pool codes shifted by one column (composition:
    conv2_2's dY)."""
    st, img, gt, rec = _native_step_capture(23, 1, 384, 512, perturb=perturb)
    fails, _ = _layer_local_errors(st, img, gt, rec)
    comp = {k for k, v in _composition_errors(st, gt, rec).items() if not _composition_ok(v)}
    if perturb == "swap_views":
        assert {"backend.2.weight", "backend.4.weight"} <= set(fails), fails.keys()
    elif perturb == "bias_row":
        assert fails and all(k.endswith(".bias") for k in fails), fails.keys()
    else:
        assert "bwd frontend.7" in comp, comp
