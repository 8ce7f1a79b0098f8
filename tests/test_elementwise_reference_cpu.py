"""CPU self-checks of tests/elementwise_reference.py: the references agree with ATen in fp64, and the bounds the GPU
tests use (tests/test_gpu_elementwise.py) have teeth: a torch fp32 emulation of the head kernels' summation order
passes them, and the same emulation with one block partial dropped, the reduce tail skipped or one et off by one bf16
ulp does not."""
import math

import pytest
import torch
import torch.nn.functional as F

import elementwise_reference as R

F64 = torch.float64
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


# ------------------------------------------------------------------------------------------- references against ATen
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,h,pitch,wv", [(2, 5, 7, 7), (1, 6, 8, 5)])
def test_head_ref_matches_autograd(dtype, n, h, pitch, wv):
    P = n * h * pitch
    y16, w, b, gt = R.head_inputs(P, dtype, seed=3)
    gscale, lscale = 0.25, 8.0
    r = R.head_ref(y16, w, b, gt, gscale, lscale, pitch, wv)
    x = y16.to(F64).view(n, h, pitch, 64).permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.to(F64).view(1, 64, 1, 1).requires_grad_(True)
    br = b.to(F64).requires_grad_(True)
    out = F.conv2d(x, wr, br)[..., :wv]
    loss = ((out - gt.to(F64).view(n, 1, h, pitch)[..., :wv]) ** 2).sum()
    gx, gw, gb = torch.autograd.grad(loss, (x, wr, br))
    et = r.et.view(n, 1, h, pitch)
    assert torch.allclose(et[..., :wv], out.detach(), rtol=1e-13, atol=1e-13)
    assert (et[..., wv:] == 0).all()
    assert math.isclose(r.loss.item(), loss.item(), rel_tol=1e-13)
    # the reference's gradients carry gscale (and dy the loss scale); autograd's are those of the plain loss
    dy = (gx.permute(0, 2, 3, 1) * (x.detach().permute(0, 2, 3, 1) > 0)).reshape(P, 64)
    assert torch.allclose(r.dy, dy * gscale * lscale, rtol=1e-12, atol=1e-13)
    assert torch.allclose(r.dw, gw.reshape(64) * gscale, rtol=1e-12, atol=1e-13)
    assert math.isclose(r.db.item(), gb.item() * gscale, rel_tol=1e-12)
    assert (r.dy.view(n, h, pitch, 64)[:, :, wv:] == 0).all()
    # the magnitude sums bound their sums
    assert (r.dw_mag >= r.dw.abs()).all() and r.db_mag >= r.db.abs() and (r.et_mag >= r.et.abs()).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("negative", [False, True], ids=["relu", "signed"])
@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_ref_forward_matches_aten(shape, negative, dtype):
    x = R.pool_input(*shape, dtype, seed=5, negative=negative)
    pooled, codes, route = R.maxpool_ref(x)
    ref = F.max_pool2d(x.to(F64).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(pooled.to(F64), ref)
    # exactly one routed element per window whose max is > 0, none elsewhere, and the code names it
    per_window = R._windows(route).sum(-1)
    assert torch.equal(per_window, (ref > 0).long())
    nib = R.unpack_codes(codes)
    assert torch.equal(nib > 0, ref > 0)
    onehot = R._windows(route).long()
    assert torch.equal((onehot * (1 << torch.arange(4))).sum(-1), nib)


@pytest.mark.parametrize("negative", [False, True], ids=["relu", "signed"])
def test_maxpool_ref_backward_matches_autograd_without_ties(negative):
    n, h, w, c = 2, 6, 10, 24
    g = torch.Generator().manual_seed(11)
    vals = (torch.randperm(n * h * w * c, generator=g).double() + 1.0) / 64.0      # all distinct: no ties
    if negative:
        vals = vals - vals.median()
    x = vals.view(n, h, w, c)
    dy = torch.randn(n, h // 2, w // 2, c, generator=g, dtype=F64)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(F.max_pool2d(xr, 2, 2), xr, dy.permute(0, 3, 1, 2))
    want = gx.permute(0, 2, 3, 1) * (x > 0)
    _, _, route = R.maxpool_ref(x)
    assert torch.equal(R.maxpool_route(route, dy), want)


def test_maxpool_ref_tie_picks_first_in_scan_order():
    for a, b in R._PAIRS:
        x = torch.full((1, 2, 2, 8), 0.25)
        x.view(-1, 8)[a] = 2.0          # rows of the [4, 8] view are the window positions (0,0),(0,1),(1,0),(1,1)
        x.view(-1, 8)[b] = 2.0
        pooled, codes, route = R.maxpool_ref(x)
        assert (pooled == 2.0).all()
        assert (R.unpack_codes(codes) == (1 << a)).all()
        assert route.view(4, 8)[a].all() and int(route.sum()) == 8
    x = torch.full((1, 2, 2, 8), 1.5)                         # all four equal: position 0
    assert (R.unpack_codes(R.maxpool_ref(x)[1]) == 1).all()
    x = torch.zeros(1, 2, 2, 8)                               # max not > 0: no code, no route
    _, codes, route = R.maxpool_ref(x)
    assert (codes == 0).all() and not route.any()


def test_code_packing_round_trips():
    g = torch.Generator().manual_seed(2)
    nib = torch.randint(0, 16, (3, 5, 7, 24), generator=g)
    nib[0, 0, 0, 7] = 8                                       # the top nibble's top bit: the word's sign bit
    codes = R.pack_codes(nib)
    assert codes.dtype == torch.int32 and codes.shape == (3, 5, 7, 3)
    assert torch.equal(R.unpack_codes(codes), nib)
    one = torch.zeros(8, dtype=torch.int64)
    one[3] = 4
    assert R.pack_codes(one).item() == 4 << 12               # channel 3 sits in nibble 3
    assert codes[0, 0, 0, 0].item() < 0


def test_split_ref_layouts_and_residual():
    x = R.split_input(37, 6, seed=1)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    assert ((x - hi.float() - lo.float()).abs() <= x.abs() * 2.0 ** -16).all()
    exact = x == hi.float()
    assert exact.any() and (lo[exact] == 0).all()
    o0 = R.split_x3_ref(x, 0, 0b100, 24)
    assert torch.equal(o0[:, 0:6], hi) and torch.equal(o0[:, 6:12], hi) and torch.equal(o0[:, 12:18], lo)
    assert (o0[:, 18:] == 0).all()
    o1 = R.split_x3_ref(x, 1, 0b010, 8)
    assert torch.equal(o1[0, :, :6], hi) and torch.equal(o1[1, :, :6], lo) and torch.equal(o1[2, :, :6], hi)
    assert (o1[:, :, 6:] == 0).all()


@pytest.mark.parametrize("name", sorted(R.SCALER_TRANSITIONS))
def test_loss_scale_ref_reproduces_expected_sequence(name):
    S, n, steps = R.SCALER_TRANSITIONS[name]
    for overflow, want in steps:
        S, inv, n = R.loss_scale_ref(S, n, overflow, **R.SCALER_ARGS)
        assert (S, inv, n) == want, (name, overflow, (S, inv, n), want)


# ------------------------------------------------------------------------------------------------- the head's bounds
def head_emulate(y16, w, b, gt, gscale, nblk, drop_block=None, skip_tail=False):
    """The head kernels' arithmetic in torch fp32, in their order of summation (products and sums rounded separately,
    where the kernels may fuse them: the emulation's error is the larger).
    head_train: lane l of a pixel's 8 holds channels 8l..8l+7 and chains their 8 products, three butterfly adds
    combine the lanes, then the bias.  Pixel p belongs to block (p // 32) % nblk, pixel group p % 32, sweep
    p // (32 nblk); a thread adds its sweeps in order, the block its 32 groups in order.
    head_reduce: group q of 15 adds blocks q, q + 30, ... into s0 and q + 15, q + 45, ... into s1 while both exist,
    one more block into s0 if one is left (skip_tail: forgotten), then s0 + s1; the 15 group sums are added in order.
    drop_block: that block's partial is left out.  Returns fp32 (et, dw [64], db, loss)."""
    P = y16.shape[0]
    v = y16.float()
    prod = (v * w.float()).view(P, 8, 8)
    s = torch.zeros(P, 8)
    for k in range(8):
        s = s + prod[:, :, k]
    for m in (1, 2, 4):
        s = s + s[:, torch.arange(8) ^ m]
    et = s[:, 0] + b.float()
    d = et - gt.float()
    g = (2.0 * d) * torch.tensor(gscale, dtype=torch.float32)
    terms = torch.cat([g[:, None] * v, g[:, None], (d * d)[:, None]], 1)            # 64 dw, db, loss
    sweep = 32 * nblk
    sweeps = math.ceil(P / sweep)
    terms = torch.cat([terms, torch.zeros(sweeps * sweep - P, 66)]).view(sweeps, nblk, 32, 66)
    thread = torch.zeros(nblk, 32, 66)
    for it in range(sweeps):
        thread = thread + terms[it]
    part = torch.zeros(nblk, 66)
    for r in range(32):
        part = part + thread[:, r]
    if drop_block is not None:
        part[drop_block] = 0.0
    G = R.REDUCE_GROUPS
    out = torch.zeros(66)
    for q in range(G):
        s0, s1, i = torch.zeros(66), torch.zeros(66), q
        while i + G < nblk:
            s0 = s0 + part[i]
            s1 = s1 + part[i + G]
            i += 2 * G
        if i < nblk and not skip_tail:
            s0 = s0 + part[i]
        out = out + (s0 + s1)
    return et, out[:64], out[64], out[65]


def _head_ratios(P, nblk, dtype, gscale=1.0, et_edit=None, **emul):
    y16, w, b, gt = R.head_inputs(P, dtype, seed=P + nblk)
    et, dw, db, loss = head_emulate(y16, w, b, gt, gscale, nblk, **emul)
    if et_edit is not None:
        et = et_edit(et)
    ref = R.head_ref(y16, w, b, gt, gscale)
    st = R.head_staged(et, y16, w, gt, gscale)
    return {"et": R.et_ratio(et, ref), "dw": R.sum_ratio(dw, st.dw, st.dw_mag, P, nblk),
            "db": R.sum_ratio(db, st.db, st.db_mag, P, nblk), "loss": R.sum_ratio(loss, st.loss, st.loss_mag, P, nblk)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P,nblk", R.HEAD_CASES)
def test_head_bounds_hold_for_fp32_emulation(P, nblk, dtype):
    r = _head_ratios(P, nblk, dtype, gscale=0.25)
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P,nblk", R.HEAD_CASES)
def test_head_bounds_notice_a_dropped_block_partial(P, nblk, dtype):
    r = _head_ratios(P, nblk, dtype, drop_block=0)            # block 0 holds pixels in every case
    assert r["dw"] > 1.0 and r["db"] > 1.0 and r["loss"] > 1.0, r


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nblk", [16, 31])
def test_head_bounds_notice_a_skipped_reduce_tail(nblk, dtype):
    r = _head_ratios(1000, nblk, dtype, skip_tail=True)
    assert r["dw"] > 1.0 and r["db"] > 1.0 and r["loss"] > 1.0, r
    assert all(v <= 1.0 for v in _head_ratios(1000, nblk, dtype).values())


@pytest.mark.parametrize("P,nblk", [(33, 2), (1000, 15)])
def test_head_et_bound_notices_one_bf16_ulp(P, nblk):
    def one_ulp(et):
        et = et.clone()
        k = P // 2
        et[k] = et[k] + 2.0 ** (math.floor(math.log2(abs(et[k].item()))) - 7)       # one bf16 ulp of et[k]
        return et
    r = _head_ratios(P, nblk, torch.bfloat16, et_edit=one_ulp)
    assert r["et"] > 1.0, r


def test_head_chain_formula():
    assert R.head_chain(1, 1) == 1 + 32 + 1 + 15 + 1
    assert R.head_chain(1000, 16) == 2 + 32 + 2 + 15 + 1
    assert R.head_chain(70001, 1024) == 3 + 32 + 69 + 15 + 1
