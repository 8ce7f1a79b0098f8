"""The memory-bound kernels of csrc/elementwise.hip, each called through its extension entry point and compared
elementwise with the plain references of tests/elementwise_reference.py: the training head (head_fwd, head_train,
head_reduce), the 2x2 max-pool and its two backwards, split_x3 (both kernels), scale_update, grad_nonfinite and
img_to_nhwc4.

Every output buffer is pre-filled with NaN (or 0xFFFF words), so an element a kernel does not write shows.  The head's
bounds are derived in elementwise_reference.py and shown on the CPU to notice one dropped block partial
(tests/test_elementwise_reference_cpu.py); everything else is exact by value or bit for bit.
"""
import math

import pytest
import torch

import elementwise_reference as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
NAN = float("nan")
_worst = {}          # (quantity, dtype, case) -> worst err / bound seen in this session
_dy_bitwise = {}     # dtype -> every dy comparison so far was exact


def _name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp16"


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module: the worst err / bound per head quantity, dtype and case (shown with ``pytest -s``)."""
    yield
    cases = list(dict.fromkeys(k[2] for k in _worst))            # in the order the tests ran
    for (q, dt, case), r in sorted(_worst.items(), key=lambda kv: (cases.index(kv[0][2]), kv[0][1], kv[0][0])):
        print(f"\nHEAD {case:<24s} {dt:<5s} {q:<5s} worst err/bound {r:.4f}", end="")
    for dt, ok in sorted(_dy_bitwise.items()):
        print(f"\nHEAD dy {dt}: {'bitwise equal to the staged fp32 reference in every case' if ok else 'NOT bitwise'}",
              end="")
    print()


@pytest.fixture(scope="module")
def ext():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require(), _ext


def _dt(dtype):
    from can_distributed_pytorch_amd.ops.conv import dt_code
    return dt_code(dtype)


def _full(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _bits(t):
    """The 16-bit words of a bf16 / fp16 tensor."""
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------- head
def _run_head(ext, y, w, b, gt, nblk, gscale, lscale, beta, pitch=0, wv=0, seed=0):
    """head_train and head_fwd on NaN-filled outputs (dw / db: random finite values when beta != 0)."""
    C, X = ext
    P = y.shape[0]
    st = X.stream_ptr()
    et, part = _full((P,), NAN), _full((nblk, 66), NAN)
    dy = _full((P, 64), NAN, y.dtype)
    loss, nonfinite = _full((1,), NAN), _full((1,), NAN)
    if beta != 0.0:
        g = torch.Generator().manual_seed(seed + 77)
        dw, db = torch.randn(64, generator=g).cuda(), torch.randn(1, generator=g).cuda()
    else:
        dw, db = _full((64,), NAN), _full((1,), NAN)
    old = (dw.clone(), db.clone())
    ls = torch.tensor([lscale], dtype=torch.float32, device="cuda") if lscale is not None else None
    C.head_train(y.data_ptr(), w.data_ptr(), b.data_ptr(), gt.data_ptr(), et.data_ptr(), dy.data_ptr(),
                 part.data_ptr(), nblk, dw.data_ptr(), db.data_ptr(), loss.data_ptr(), P, gscale, beta,
                 ls.data_ptr() if ls is not None else 0, nonfinite.data_ptr(), _dt(y.dtype), st, pitch, wv)
    et_fwd = _full((P,), NAN)
    C.head_fwd(y.data_ptr(), w.data_ptr(), b.data_ptr(), et_fwd.data_ptr(), P, _dt(y.dtype), st, pitch, wv)
    torch.cuda.synchronize()
    return dict(et=et, et_fwd=et_fwd, dy=dy, dw=dw, db=db, loss=loss, nonfinite=nonfinite, part=part, old=old)


def _check_head(o, y, w, b, gt, nblk, gscale, lscale, beta, case, pitch=0, wv=0):
    """All of the head's checks on one run; returns the failures (empty: passed)."""
    P, dt = y.shape[0], _name(y.dtype)
    failed = []

    def note(q, ratio):
        key = (q, dt, case)
        _worst[key] = max(_worst.get(key, 0.0), ratio)
        if not ratio <= 1.0:
            failed.append(f"{case} {dt} {q}: err / bound = {ratio:.4g} (gscale {gscale}, lscale {lscale}, beta {beta})")

    ref = R.head_ref(y, w, b, gt, gscale, lscale, pitch, wv)
    note("et", R.et_ratio(o["et"], ref))
    if not torch.equal(o["et_fwd"].view(torch.int32), o["et"].view(torch.int32)):
        failed.append(f"{case} {dt}: head_fwd's et is not head_train's bit for bit")
    if not bool(torch.isfinite(o["part"]).all()):
        failed.append(f"{case} {dt}: a block partial was not written")
    st = R.head_staged(o["et"], y, w, gt, gscale, lscale, pitch, wv)
    same = torch.equal(_bits(o["dy"]), _bits(st.dy))              # the 16-bit words: the sign of a zero included
    _dy_bitwise[dt] = _dy_bitwise.get(dt, True) and same
    if not same:
        bad = int((o["dy"].float() != st.dy.float()).sum())
        failed.append(f"{case} {dt}: dy differs from the staged fp32 reference at {bad} elements")
    if not bool((o["dy"].float()[~st.valid] == 0).all() and (o["et"][~st.valid] == 0).all()):
        failed.append(f"{case} {dt}: et / dy not 0 at a padding pixel")
    note("dw", R.sum_ratio(o["dw"], st.dw, st.dw_mag, P, nblk, beta, o["old"][0]))
    note("db", R.sum_ratio(o["db"], st.db, st.db_mag, P, nblk, beta, o["old"][1]))
    note("loss", R.sum_ratio(o["loss"], st.loss, st.loss_mag, P, nblk))
    if o["nonfinite"].item() != 0.0:
        failed.append(f"{case} {dt}: nonfinite = {o['nonfinite'].item()} for a finite loss")
    return failed


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P,nblk", R.HEAD_CASES)
def test_head_train_fwd_elementwise(ext, P, nblk, dtype):
    """et against fp64 within 2 * 12 * 2^-24 (sum|y w| + |b|); head_fwd == head_train's et bit for bit; dy bit for bit
    the fp32 staging on the kernel's own et (the kernel's dy has no addition, so no contraction can change it: no ulp
    allowance is made); dw, db, loss within 2 L 2^-24 sum|terms| of the fp64 sums of the staged fp32 g (+ the beta
    term's 2^-23 (|beta old| + |sum|)), L = elementwise_reference.head_chain.  Measured ratios: profiles/r12."""
    y, w, b, gt = R.head_inputs(P, dtype, seed=1000 + P + nblk, device="cuda")
    failed = []
    for gscale, lscale, beta in R.HEAD_CONFIGS:
        o = _run_head(ext, y, w, b, gt, nblk, gscale, lscale, beta, seed=P)
        failed += _check_head(o, y, w, b, gt, nblk, gscale, lscale, beta, f"P={P} nblk={nblk}")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P,nblk", [(33, 2), (1000, 16)])
def test_head_nonfinite_flag(ext, P, nblk, dtype):
    """One gt = inf: the loss is inf and the flag 1.0 (0.0 for the finite loss: _check_head); dw / db are whatever the
    sums give."""
    y, w, b, gt = R.head_inputs(P, dtype, seed=5 + P, device="cuda")
    gt[P // 3] = float("inf")
    o = _run_head(ext, y, w, b, gt, nblk, 1.0, None, 0.0)
    assert o["loss"].item() == float("inf")
    assert o["nonfinite"].item() == 1.0
    assert not torch.isnan(o["et"]).any() and torch.equal(o["et_fwd"], o["et"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,pitch,wv", R.HEAD_PADDED)
def test_head_width_padding(ext, rows, pitch, wv, dtype):
    """Padding columns hold y = 3.0 and gt = 1e6: et and dy are exactly 0 there, and loss, dw, db are those of the
    valid pixels alone (the references mask the padding), within the bounds of test_head_train_fwd_elementwise."""
    P = rows * pitch
    nblk = math.ceil(P / 32)
    y, w, b, gt = R.head_inputs(P, dtype, seed=31 + P, device="cuda")
    pad = ~R.head_valid(P, pitch, wv, "cuda")
    y[pad] = 3.0
    gt[pad] = 1e6
    failed = []
    for gscale, lscale, beta in R.HEAD_CONFIGS[:2]:
        o = _run_head(ext, y, w, b, gt, nblk, gscale, lscale, beta, pitch, wv, seed=P)
        failed += _check_head(o, y, w, b, gt, nblk, gscale, lscale, beta, f"rows={rows} pitch={pitch} wv={wv}",
                              pitch, wv)
    assert not failed, "\n".join(failed)


@pytest.fixture(scope="module", params=DTYPES, ids=IDS)
def executor(request):
    from can_distributed_pytorch_amd.models import CANNet
    from can_distributed_pytorch_amd.ops.executor import CANNetExecutor
    torch.manual_seed(2)
    model = CANNet().cuda()
    torch.nn.init.normal_(model.output_layer.weight, std=0.1)
    torch.nn.init.constant_(model.output_layer.bias, 0.3)
    return CANNetExecutor(model, dtype=request.param)


@pytest.mark.parametrize("n,h,w", [(2, 9, 14), (1, 160, 250)])
def test_head_train_through_executor(executor, n, h, w):
    """CANNetExecutor.head_train: its own nblk = min(1024, ceil(P / 32)), the loss and its flag in ``flags``, beta."""
    ex = executor
    P = n * h * w
    nblk = max(1, min(1024, math.ceil(P / 32)))
    y, _, _, gt = R.head_inputs(P, ex.act, seed=400 + P, device="cuda")
    wt = ex.head.weight.detach().reshape(64)
    b = ex.head.bias.detach()
    torch.manual_seed(P)
    failed = []
    for gscale, lscale, beta in R.HEAD_CONFIGS:
        grads = [None] * ex.n_params
        if beta != 0.0:
            grads[ex.head_w_index] = torch.randn(1, 64, 1, 1, device="cuda")
            grads[ex.head_b_index] = torch.randn(1, device="cuda")
        else:
            grads[ex.head_w_index] = _full((1, 64, 1, 1), NAN)
            grads[ex.head_b_index] = _full((1,), NAN)
        old = (grads[ex.head_w_index].clone(), grads[ex.head_b_index].clone())
        flags = _full((4,), NAN)
        ls = torch.tensor([lscale], dtype=torch.float32, device="cuda") if lscale is not None else None
        loss, et, dy = ex.head_train(y.view(n, h, w, 64), gt.view(n, 1, h, w), grads, gscale=gscale, beta=beta,
                                     lscale=ls, flags=flags)
        et_fwd = _full((P,), NAN)
        ex.C.head_fwd(y.data_ptr(), wt.data_ptr(), b.data_ptr(), et_fwd.data_ptr(), P, ex.dt, ex._stream(), 0, 0)
        torch.cuda.synchronize()
        assert loss.data_ptr() == flags[1:2].data_ptr() and torch.isnan(flags[2:]).all()
        o = dict(et=et.reshape(P), et_fwd=et_fwd, dy=dy.reshape(P, 64), dw=grads[ex.head_w_index],
                 db=grads[ex.head_b_index], loss=flags[1:2], nonfinite=flags[0:1], part=torch.zeros(1, device="cuda"),
                 old=old)
        failed += _check_head(o, y, wt, b, gt, nblk, gscale, lscale, beta, f"executor n={n} h={h} w={w}")
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------------------------------------------------- max-pool
def _run_pool(ext, x, dy):
    """(pooled, codes, pooled without codes, dx from the codes, dx from x), every output pre-filled."""
    C, X = ext
    n, h, w, c = x.shape
    st, dt = X.stream_ptr(), _dt(x.dtype)
    y = _full((n, h // 2, w // 2, c), NAN, x.dtype)
    y2 = _full((n, h // 2, w // 2, c), NAN, x.dtype)
    codes = _full((n, h // 2, w // 2, c // 8), 0x7ABCDEF0, torch.int32)
    C.maxpool_fwd(x.data_ptr(), y.data_ptr(), n, h, w, c, dt, st, codes.data_ptr())
    C.maxpool_fwd(x.data_ptr(), y2.data_ptr(), n, h, w, c, dt, st)
    dx1, dx2 = _full(x.shape, NAN, x.dtype), _full(x.shape, NAN, x.dtype)
    C.maxpool_bwd_codes(codes.data_ptr(), dy.data_ptr(), dx1.data_ptr(), n, h, w, c, dt, st)
    C.maxpool_bwd_relu(x.data_ptr(), dy.data_ptr(), dx2.data_ptr(), n, h, w, c, dt, st)
    torch.cuda.synchronize()
    return y, codes, y2, dx1, dx2


def _check_pool(ext, shape, dtype, negative):
    n, h, w, c = shape
    torch.manual_seed(n * h * w + c)
    x = R.pool_input(n, h, w, c, dtype, seed=17 + c, negative=negative, device="cuda")
    dy = (torch.randn(n, h // 2, w // 2, c, device="cuda") + 3.0).to(dtype)       # no zeros: a dropped route shows
    y, codes, y2, dx1, dx2 = _run_pool(ext, x, dy)
    pooled, rcodes, route = R.maxpool_ref(x)
    want = R.maxpool_route(route, dy)
    assert torch.equal(y, pooled), "pooled values"
    assert torch.equal(y2, pooled), "pooled values without the codes argument"
    assert torch.equal(codes, rcodes), "codes"
    assert torch.equal(dx1, want), "maxpool_bwd_codes"
    assert torch.equal(dx2, want), "maxpool_bwd_relu"
    if negative:
        assert bool((R.unpack_codes(codes)[pooled <= 0] == 0).all())
        assert bool((pooled <= 0).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("negative", [False, True], ids=["relu", "signed"])
@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_three_kernels_exact(ext, shape, negative, dtype):
    _check_pool(ext, shape, dtype, negative)


def _pool_items(shape):
    n, h, w, c = shape
    return n * (h // 2) * (w // 2) * (c // 8)


def test_maxpool_full_grid(ext):
    """Exactly as many vector items as the capped grid has threads (8192 blocks of 256): one sweep, no thread idle."""
    assert _pool_items(R.POOL_FULL_GRID) == R.POOL_GRID_ITEMS
    _check_pool(ext, R.POOL_FULL_GRID, torch.bfloat16, False)


def test_maxpool_second_grid_sweep(ext):
    """8192 items more than the capped grid has threads: the first 32 blocks' threads take a second item (the
    grid-stride step), the others do not (a ragged second sweep)."""
    assert R.POOL_GRID_ITEMS < _pool_items(R.POOL_TWO_SWEEPS) < 2 * R.POOL_GRID_ITEMS
    _check_pool(ext, R.POOL_TWO_SWEEPS, torch.float16, False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(1, 3, 4, 8), (1, 4, 5, 8), (1, 4, 4, 12)], ids=["odd_h", "odd_w", "c_12"])
def test_maxpool_refuses_odd_shapes(ext, shape, dtype):
    C, X = ext
    n, h, w, c = shape
    st, dt = X.stream_ptr(), _dt(dtype)
    x = torch.ones(n, h + 1, w + 1, 16, dtype=dtype, device="cuda")               # larger than any reading of the shape
    dy = torch.ones_like(x)
    out = _full(x.shape, NAN, dtype)
    codes = _full((x.numel(),), 0x7ABCDEF0, torch.int32)
    with pytest.raises(RuntimeError, match="rc=-2"):
        C.maxpool_fwd(x.data_ptr(), out.data_ptr(), n, h, w, c, dt, st, codes.data_ptr())
    with pytest.raises(RuntimeError, match="rc=-2"):
        C.maxpool_bwd_codes(codes.data_ptr(), dy.data_ptr(), out.data_ptr(), n, h, w, c, dt, st)
    with pytest.raises(RuntimeError, match="rc=-2"):
        C.maxpool_bwd_relu(x.data_ptr(), dy.data_ptr(), out.data_ptr(), n, h, w, c, dt, st)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and bool((codes == 0x7ABCDEF0).all())


# ---------------------------------------------------------------------------------------------------------- split_x3
@pytest.mark.parametrize("pattern", R.SPLIT_PATTERNS, ids=lambda p: f"pat{p:03b}")
@pytest.mark.parametrize("M", R.SPLIT_M)
@pytest.mark.parametrize("C_,stride,mode", R.SPLIT_VEC + R.SPLIT_GENERAL)
def test_split_x3_bitwise(ext, C_, stride, mode, M, pattern):
    """Bit for bit against split_x3_ref through ops.fp32.split_x3 and through the raw entry point.  Only the raw call
    shows that the zero padding columns are written: its buffer holds 0xFFFF words, while ops.fp32.split_x3 allocates
    its own output (torch.empty); both launch the same kernel."""
    from can_distributed_pytorch_amd.ops import fp32
    C, X = ext
    x = R.split_input(M, C_, seed=M + C_, device="cuda")
    want = R.split_x3_ref(x, mode, pattern, stride)
    got = fp32.split_x3(x.view(1, 1, M, C_), mode, pattern, stride=stride)
    torch.cuda.synchronize()
    assert got.shape == ((1, 1, M, stride) if mode == 0 else (3, 1, M, stride))
    assert torch.equal(_bits(got).reshape(-1), _bits(want).reshape(-1))
    raw = _full(tuple(want.shape), -1, torch.int16)
    C.split_x3(x.data_ptr(), raw.data_ptr(), M, C_, stride, mode, pattern, X.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(raw.reshape(-1), _bits(want).reshape(-1))


def test_split_x3_refuses_bad_arguments(ext):
    C, X = ext
    x = torch.ones(8, 8, device="cuda")
    out = _full((3 * 8 * 64,), -1, torch.int16)
    for (c, stride, mode) in [(8, 16, 0), (8, 4, 1), (8, 24, 2), (8, 24, -1)]:
        with pytest.raises(RuntimeError, match="rc=-2"):
            C.split_x3(x.data_ptr(), out.data_ptr(), 8, c, stride, mode, 0, X.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == -1).all())


# ------------------------------------------------------------------------------------------------------ scale_update
@pytest.mark.parametrize("name", sorted(R.SCALER_TRANSITIONS))
def test_scale_update_state_machine(ext, name):
    """After every launch {S, 1/S, n} equals loss_scale_ref (and the hand-written expectation) exactly."""
    C, X = ext
    S, n, steps = R.SCALER_TRANSITIONS[name]
    scaler = torch.tensor([S, 1.0 / S, n, 7.0], dtype=torch.float32, device="cuda")
    flag = torch.zeros(1, dtype=torch.float32, device="cuda")
    a = R.SCALER_ARGS
    for k, (overflow, want) in enumerate(steps):
        flag.fill_(float(overflow))
        C.scale_update(flag.data_ptr(), scaler.data_ptr(), a["interval"], a["growth"], a["backoff"], a["max_scale"],
                       X.stream_ptr())
        torch.cuda.synchronize()
        S, inv, n = R.loss_scale_ref(S, n, overflow, **a)
        got = tuple(scaler[:3].tolist())
        assert got == (S, inv, n) == want, (name, k, got, (S, inv, n), want)
        assert scaler[3].item() == 7.0 and flag.item() == float(overflow)


# ---------------------------------------------------------------------------------------------------- grad_nonfinite
GN = 4 * (2048 * 256) + 4 * 1000       # one float4 sweep of the 2048-block grid and a ragged second one


def _nonfinite_flag(ext, g, start):
    C, X = ext
    flag = torch.tensor([start], dtype=torch.float32, device="cuda")
    C.grad_nonfinite(g.data_ptr(), g.numel(), flag.data_ptr(), X.stream_ptr())
    torch.cuda.synchronize()
    return flag.item()


@pytest.fixture(scope="module")
def clean_grad():
    g = torch.randn(GN, device="cuda")
    g[5] = 3.0e38
    g[GN - 7] = -3.0e38
    g[9] = 1e-40                        # a denormal
    g[4 * 2048 * 256 + 11] = -1e-45
    return g


def test_grad_nonfinite_clean_buffer(ext, clean_grad):
    assert torch.isfinite(clean_grad).all()
    assert _nonfinite_flag(ext, clean_grad, 0.0) == 0.0
    assert _nonfinite_flag(ext, clean_grad, 1.0) == 1.0


@pytest.mark.parametrize("where", [0, GN - 1, 4 * 2048 * 256 + 4 * 500 + 1], ids=["first", "last", "second_sweep"])
@pytest.mark.parametrize("value", [float("inf"), float("-inf"), NAN], ids=["inf", "neg_inf", "nan"])
def test_grad_nonfinite_one_bad_element(ext, clean_grad, value, where):
    g = clean_grad.clone()
    g[where] = value
    assert _nonfinite_flag(ext, g, 0.0) == 1.0
    assert _nonfinite_flag(ext, g, 1.0) == 1.0


def test_grad_nonfinite_refuses_ragged_count(ext, clean_grad):
    C, X = ext
    flag = torch.zeros(1, device="cuda")
    bad = clean_grad[:1026].clone()
    bad[1025] = NAN
    with pytest.raises(RuntimeError, match="rc=-2"):
        C.grad_nonfinite(bad.data_ptr(), 1026, flag.data_ptr(), X.stream_ptr())
    torch.cuda.synchronize()
    assert flag.item() == 0.0


# ------------------------------------------------------------------------------------------------------ img_to_nhwc4
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,h,w", [(2, 5, 7), (1, 1, 1), (3, 64, 96), (1, 1500, 1500)])
def test_img_to_nhwc4_bitwise(ext, n, h, w, dtype):
    """Bit for bit the torch conversion (ops.conv.to_nhwc4), channel 3 zero, on an output of NaN bits; 1500 x 1500 has
    more pixels than the 8192-block grid covers in one sweep.  The three channels hold different values, so a channel
    swap cannot pass."""
    from can_distributed_pytorch_amd.ops.conv import to_nhwc4
    C, X = ext
    torch.manual_seed(n * h + w)
    img = torch.randn(n, 3, h, w, device="cuda") * torch.tensor([1.0, 37.0, 1e-3], device="cuda").view(1, 3, 1, 1)
    img.view(-1)[::7] *= 1e5            # past fp16's range now and then
    out = _full((n, h, w, 4), NAN, dtype)
    C.img_to_nhwc4(img.data_ptr(), out.data_ptr(), n, h, w, _dt(dtype), X.stream_ptr())
    torch.cuda.synchronize()
    want = to_nhwc4(img, dtype)
    assert torch.equal(_bits(out), _bits(want))
    assert bool((_bits(out)[..., 3] == 0).all())
    for ch in range(3):                 # against the definition, not only the helper
        assert torch.equal(_bits(out[..., ch]), _bits(img[:, ch].to(dtype)))
