"""The context module's kernels stage by stage against the staged fp64 reference (tests/ctx_reference.py).

Teacher forcing: every stage is fed the kernel's own upstream output and compared with the reference of that ONE stage
on the same values, so errors do not compound and a failure names its stage.  The bounds are the project's elementwise
defaults (tests/numerics.py check_out16 / check_sum32, zero outliers; the pooled cells their own summation bound,
ctx_reference.pool_bound); tests/test_ctx_reference_cpu.py proves on the CPU that the rounded reference alone meets
them on these inputs and that a one-pixel mistake in any geometric step does not.

Storage points the reference follows (read off the kernels):
  * linear form (conv_igemm.hip EPI_CTXF): t = W2 u comes from the fp32 master weights (ctx_gemm), G = W2 fv from the
    16-bit pack; fi is formed from the fp32 sigmoid values, so its reference uses the reference's own w;
  * direct form (context.hip ctx_fuse / ctx_bwd_e1): fi, dz and sdir are formed from the stored 16-bit w, so their
    reference reads the kernel's w;
  * both backwards (ctx_bwd_lin, ctx_bwd_e1) read the stored 16-bit w and recompute s and fi from the cell table;
  * the eight weight gradients (stages dW1 / dW2) come from the executor's own _context_bwd, so the schedule is under
    test too: linear form dW1_S = du_all_S^T ave_S and dW2_S = dG_S^T fv + dt_S^T u_S from the stored 16-bit dG and
    the fp32 cell tables, direct form dW1_S = dA_S^T ave_S and dW2_S = dz_S^T cs_S, each beta g0 + scale dscale (...)
    at the settings of ctx_reference.WGRAD_SETTINGS.  tests/test_ctx_reference_cpu.py proves that the check sees a
    dropped, flipped, misplaced, doubly accumulated or wrongly scaled term and misread cell tables.
"""
import types

import pytest
import torch

import ctx_reference as R
from ctx_reference import SCALES
from numerics import check_out16, check_sum32

pytestmark = pytest.mark.gpu

C = 512
_worst = {}          # (stage, dtype) -> worst err / bound seen in this session


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module: the worst err / bound per stage and dtype (shown with ``pytest -s``)."""
    yield
    for (stage, dt), r in sorted(_worst.items()):
        print(f"\nCTX-STAGE {stage:<22s} {dt:<5s} worst err/bound {r:.4f}", end="")
    print()


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def ctx(request):
    from can_distributed_pytorch_amd.models import CANNet
    from can_distributed_pytorch_amd.ops.executor import CANNetExecutor
    dtype = request.param
    torch.manual_seed(1234)
    model = CANNet(backend="hip").cuda()
    with torch.no_grad():
        for s in SCALES:
            getattr(model, f"conv{s}_1").weight.normal_(0, 0.05)
            getattr(model, f"conv{s}_2").weight.normal_(0, 0.05)
    ex = CANNetExecutor(model, dtype=dtype)
    ex.refresh_packs(force=True)
    torch.cuda.synchronize()
    W1 = torch.stack([getattr(model, f"conv{s}_1").weight.detach().view(C, C) for s in SCALES]).double()
    # the 16-bit conv{S}_2 values the packs hold: the interleaved pack (rows 4c + si) and the per-scale one
    W2cat = ex.ctx2cat_fwd.double().view(C, 4, C).permute(1, 0, 2).contiguous()
    W2dir = ex.ctx2_fwd.double()
    return types.SimpleNamespace(ex=ex, model=model, dtype=dtype, name="bf16" if dtype == torch.bfloat16 else "fp16",
                                 W1=W1, W2cat=W2cat, W2dir=W2dir)


class Checks:
    """Runs every stage check of a case, then fails with all that missed (the stages are independent)."""

    def __init__(self, cx, form):
        self.cx, self.form, self.failed = cx, form, []

    def _note(self, stage, ratio, detail=""):
        key = (f"{self.form}/{stage}", self.cx.name)
        _worst[key] = max(_worst.get(key, 0.0), ratio)
        if not ratio <= 1.0:
            self.failed.append(f"{key[0]}: err / bound = {ratio:.4g} {detail}")

    def out16(self, stage, got, ref):
        detail = ""
        try:
            check_out16(got, ref.float(), what=stage)
        except AssertionError as e:
            detail = str(e)
        self._note(stage, max(R.out16_ratio(got, ref), 2.0 if detail else 0.0), detail)

    def cells32(self, stage, got, ref):
        detail = ""
        try:
            for S, o in zip(SCALES, R.CELL_OFF):
                check_sum32(got[:, o:o + S * S], ref[:, o:o + S * S].float(), what=f"{stage}, scale {S}")
        except AssertionError as e:
            detail = str(e)
        self._note(stage, max(R.cells_sum32_ratio(got, ref), 2.0 if detail else 0.0), detail)

    def wgrad32(self, stage, got, ref):
        """The four scales' weight gradients [4, C, C]: check_sum32 at its default tolerance, scale by scale."""
        detail = ""
        try:
            for si, S in enumerate(SCALES):
                check_sum32(got[si], ref[si].float(), what=f"{stage}, scale {S}")
        except AssertionError as e:
            detail = str(e)
        self._note(stage, max(R.wgrad_sum32_ratio(got, ref), 2.0 if detail else 0.0), detail)

    def pool(self, stage, got, fv, geo):
        self._note(stage, R.pool_ratio(got, fv, geo))

    def equal(self, stage, got, ref):
        if not torch.equal(got, ref):
            self.failed.append(f"{self.form}/{stage}: not bitwise equal")

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def _inputs(n, h, w, dtype, seed):
    fv = R.structured_fv(n, h, w, C, dtype, seed, device="cuda")
    g = torch.Generator().manual_seed(seed + 1)
    dcat = torch.randn(n, h, w, 2 * C, generator=g).to(dtype).cuda()
    dave = torch.randn(n, 50, C, generator=g).cuda()
    return fv, dcat, dave


def _scales_first(x, n, h, w):
    """[N, h, w, 4C] with columns 4c + si -> [4, N, h, w, C]."""
    return x.reshape(n, h, w, C, 4).permute(4, 0, 1, 2, 3)


# ---------------------------------------------------------------------------------------------------------- linear form
def _kernels_linear(cx, fv, dcat, dave_r, wv=None):
    """Every kernel of the linearised form, forward and backward, as ops/context_exec.py chains them."""
    from can_distributed_pytorch_amd.ops import conv as CV
    ex = cx.ex
    n, h, w, c = fv.shape
    st = ex._stream()
    cat, sv = ex._context_fwd_linear(fv, True, wv)
    u = sv["u"]
    t = torch.empty_like(u)               # not saved by the forward: the same launch again (fixed-order, bitwise)
    ex.C.ctx_gemm(0, u.data_ptr(), 0, ex._ctx2_ptrs(), t.data_ptr(), [], n, c, 0.0, 1.0, 0, st)
    dg, rowacc = CV.ctx_bwd_lin(dcat, sv["wts"], u, wvalid=wv)
    dt = torch.empty(n, 50, c, dtype=torch.float32, device=fv.device)
    du = torch.empty_like(dt)
    ex.C.ctx_cells(rowacc[0].data_ptr(), dt.data_ptr(), n, h, c, st, rowacc[1].data_ptr(), du.data_ptr())
    du_all = du.clone()
    ex.C.ctx_gemm(1, dt.data_ptr(), 0, ex._ctx2_ptrs(), du_all.data_ptr(), [], n, c, 1.0, 1.0, 0, st)
    dave = torch.empty_like(du)
    ex.C.ctx_gemm(1, du_all.data_ptr(), 0, ex._ctx1_ptrs(), dave.data_ptr(), [], n, c, 0.0, 1.0, 0, st)
    dfv = CV.conv_ctx_bwd(dg, ex.ctx2cat_dgr, dave, dcat, fv, wvalid=wv)
    dcat0 = dcat.clone()
    dcat0[..., :c] = 0
    dfv_pool = CV.conv_ctx_bwd(torch.zeros_like(dg), ex.ctx2cat_dgr, dave_r, dcat0, fv, wvalid=wv)
    torch.cuda.synchronize()
    return dict(ave=sv["ave"], u=u, t=t, wts=sv["wts"], cat=cat, dg=dg, dt=dt, du=du, du_all=du_all, dave=dave,
                dfv=dfv, dfv_pool=dfv_pool, saved=sv)


def _check_linear(cx, k, fv, dcat, dave_r):
    """fv, dcat and the maps of ``k`` at their valid columns."""
    n, h, w, c = fv.shape
    geo = R.Geometry(h, w, fv.device)
    ck = Checks(cx, "linear")
    ck.pool("ave", k["ave"], fv, geo)
    w_ref, fi_ref, _ = R.weights_and_fi(fv, k["u"], k["t"], cx.W2cat, geo)
    wk = _scales_first(k["wts"], n, h, w)
    ck.out16("w", wk, w_ref)
    ck.out16("fi", k["cat"][..., c:], fi_ref)
    ck.equal("fv copy", k["cat"][..., :c], fv)
    dz, ds = R.bwd_pointwise(dcat[..., c:], wk, R.upsample(k["u"], geo))
    dgk = _scales_first(k["dg"], n, h, w)
    ck.out16("dg", dgk, -dz)
    ck.cells32("dt", k["dt"], R.upsample_adjoint(dz, geo))
    ck.cells32("du", k["du"], R.upsample_adjoint(ds, geo))
    ck.out16("dfv, pool^T only", k["dfv_pool"], R.pool_adjoint(dave_r, geo) * (fv.double() > 0))
    ck.out16("dfv", k["dfv"], R.dfv_linear(dgk, cx.W2cat, dcat[..., :c], k["dave"], fv, geo))
    ck.done()


@pytest.mark.parametrize("tile", [256, 128])
@pytest.mark.parametrize("n,h,w", [s for s in R.LINEAR_SHAPES if s[1] >= 3])
def test_linear_stages(ctx, dispatch_cfg, n, h, w, tile):
    dispatch_cfg(ctx_linear=1, ctx_tile_f=tile, ctx_tile_b=tile)
    fv, dcat, dave_r = _inputs(n, h, w, ctx.dtype, seed=1000 * h + w)
    assert ctx.ex._ctx_linear(fv)
    _check_linear(ctx, _kernels_linear(ctx, fv, dcat, dave_r), fv, dcat, dave_r)


@pytest.mark.parametrize("tile", [256, 128])
def test_linear_stages_width_padded(ctx, dispatch_cfg, tile):
    """A 127-column map at a row pitch of 128: every stage against the reference of the 127-column map at the valid
    columns, and zero beyond them (w, cat, dG and dfv)."""
    n, h, w = R.PADDED_SHAPE
    pitch = 128
    dispatch_cfg(ctx_linear=1, ctx_tile_f=tile, ctx_tile_b=tile)
    fv, dcat, dave_r = _inputs(n, h, w, ctx.dtype, seed=1000 * h + w)
    fvp = torch.zeros(n, h, pitch, C, dtype=ctx.dtype, device="cuda")
    fvp[:, :, :w] = fv
    dcatp = torch.zeros(n, h, pitch, 2 * C, dtype=ctx.dtype, device="cuda")
    dcatp[:, :, :w] = dcat
    k = _kernels_linear(ctx, fvp, dcatp, dave_r, wv=w)
    for name in ("wts", "cat", "dg", "dfv", "dfv_pool"):
        assert not bool(k[name][:, :, w:].any()), f"{name} is not zero at the padding columns"
        k[name] = k[name][:, :, :w]
    _check_linear(ctx, k, fv, dcat, dave_r)


# ---------------------------------------------------------------------------------------------------------- direct form
def _kernels_direct(cx, fv, dcat, dave_r):
    """Every kernel of the direct form, forward and backward, as ops/context_exec.py chains them."""
    from can_distributed_pytorch_amd.ops import conv as CV
    ex = cx.ex
    n, h, w, c = fv.shape
    st = ex._stream()
    cat, sv = ex._context_fwd(fv, True)
    assert not sv.get("linear", False)
    dz = torch.empty(4, n, h, w, c, dtype=cx.dtype, device=fv.device)
    sdir = torch.empty_like(dz)
    ex.C.ctx_bwd_e1(dcat.data_ptr(), sv["wts"].data_ptr(), sv["table"].data_ptr(), dz.data_ptr(), sdir.data_ptr(),
                    n, h, w, c, ex.dt, st)
    dc = torch.empty_like(dz)
    if ex._ctx_batched(h, w):
        CV.conv_igemm_batched(dz, ex.ctx2_dgr, ksize=1, epi=CV.EPI_NONE, out=dc)
    else:
        for i in range(4):
            CV.conv_igemm(dz[i], ex.ctx2_dgr[i], None, ksize=1, epi=CV.EPI_NONE, out=dc[i])
    dA = torch.empty(n, 50, c, dtype=torch.float32, device=fv.device)
    ex.C.ctx_reduce(1, 0, sdir.data_ptr(), dc.data_ptr(), sv["rowacc"].data_ptr(), dA.data_ptr(), n, h, w, c, ex.dt,
                    st)
    dave = torch.empty_like(dA)
    ex.C.ctx_gemm(1, dA.data_ptr(), 0, ex._ctx1_ptrs(), dave.data_ptr(), [], n, c, 0.0, 1.0, 0, st)
    dfv = torch.empty_like(fv)
    ex.C.ctx_bwd_final(dcat.data_ptr(), dc.data_ptr(), dave.data_ptr(), fv.data_ptr(), dfv.data_ptr(), n, h, w, c,
                       ex.dt, st)
    dcat0 = dcat.clone()
    dcat0[..., :c] = 0
    dfv_pool = torch.empty_like(fv)
    ex.C.ctx_bwd_final(dcat0.data_ptr(), torch.zeros_like(dc).data_ptr(), dave_r.data_ptr(), fv.data_ptr(),
                       dfv_pool.data_ptr(), n, h, w, c, ex.dt, st)
    torch.cuda.synchronize()
    return dict(ave=sv["ave"], table=sv["table"], cs=sv["cs"], wts=sv["wts"], cat=cat, dz=dz, sdir=sdir, dc=dc, dA=dA,
                dave=dave, dfv=dfv, dfv_pool=dfv_pool, saved=sv)


def _check_direct(cx, k, fv, dcat, dave_r):
    n, h, w, c = fv.shape
    geo = R.Geometry(h, w, fv.device)
    ck = Checks(cx, "direct")
    ck.pool("ave", k["ave"], fv, geo)
    ck.out16("c", k["cs"], R.direct_c(k["table"], fv, geo))
    ck.out16("w", k["wts"], torch.sigmoid(R.conv1x1_maps(k["cs"], cx.W2dir)))
    s = R.upsample(k["table"], geo)
    ck.out16("fi", k["cat"][..., c:], R.fuse(k["wts"], s))
    ck.equal("fv copy", k["cat"][..., :c], fv)
    dz, sdir = R.bwd_pointwise(dcat[..., c:], k["wts"], s)
    ck.out16("dz", k["dz"], dz)
    ck.out16("sdir", k["sdir"], sdir)
    ck.cells32("dA", k["dA"], R.upsample_adjoint(k["sdir"].double() + k["dc"].double(), geo))
    ck.out16("dfv, pool^T only", k["dfv_pool"], R.pool_adjoint(dave_r, geo) * (fv.double() > 0))
    ck.out16("dfv", k["dfv"], R.dfv_direct(k["dc"], dcat[..., :c], k["dave"], fv, geo))
    ck.done()


@pytest.mark.parametrize("n,h,w", [s for s in R.DIRECT_SHAPES if min(s[1:]) >= 2])
def test_direct_stages(ctx, dispatch_cfg, n, h, w):
    if w >= 64:
        dispatch_cfg(ctx_linear=0)
    fv, dcat, dave_r = _inputs(n, h, w, ctx.dtype, seed=1000 * h + w)
    assert not ctx.ex._ctx_linear(fv)
    _check_direct(ctx, _kernels_direct(ctx, fv, dcat, dave_r), fv, dcat, dave_r)


@pytest.mark.parametrize("n,h,w", [(2, 2, 67), (1, 2, 64)])
def test_linear_form_refuses_fewer_than_3_rows(ctx, dispatch_cfg, n, h, w):
    """ops.conv.conv_ctx_fwd / conv_ctx_bwd raise ValueError below 3 rows: the EPI_CTXB epilogue's pooling adjoint
    adds at most two row bins per scale at a pixel, and below 3 rows the bins of the 3- and 6-grids repeat
    (tests/test_ctx_reference_cpu.py test_pool_bins_overlap_at_most_two_from_length_3).  With the default dispatch
    the executor runs such a map through the direct form, checked here stage by stage, and does not pad its width."""
    from can_distributed_pytorch_amd.ops import conv as CV
    ex = ctx.ex
    dispatch_cfg(ctx_linear=1)
    fv, dcat, dave_r = _inputs(n, h, w, ctx.dtype, seed=1000 * h + w)
    cells = torch.zeros(n, 50, C, device="cuda")
    with pytest.raises(ValueError):
        CV.conv_ctx_fwd(fv, ex.ctx2cat_fwd, cells, cells)
    with pytest.raises(ValueError):
        CV.conv_ctx_bwd(torch.zeros(n, h, w, 4 * C, dtype=ctx.dtype, device="cuda"), ex.ctx2cat_dgr, cells, dcat, fv)
    assert not ex._ctx_linear(fv)
    assert ex.padded_width(8 * w + 8, 8 * h) == 8 * w + 8
    _check_direct(ctx, _kernels_direct(ctx, fv, dcat, dave_r), fv, dcat, dave_r)


@pytest.mark.parametrize("n,h,w", [s for s in R.LINEAR_SHAPES + R.DIRECT_SHAPES if min(s[1:]) < 2])
def test_one_row_or_one_column_maps_are_refused(ctx, dispatch_cfg, n, h, w):
    """(1, 1, 64) of the linear shapes and (1, 1, 5), (2, 5, 1) of the direct ones are refused on the host, before
    any launch of the refusing call: the linear wrappers raise ValueError below 3 rows (see above), and the direct
    form's conv{S}_2 GEMMs go through ops.conv.conv_igemm, whose kernels need a map of at least 2 x 2 (rc = -7;
    the batched launch is not used below 2 x 2 either, context_exec._ctx_batched).  The executor cannot reach the
    context module with such a map: conv4_3, the layer that produces fv, refuses it in the same way, so an image
    of 8 rows or 8 columns (which the trainer's --crop-size would accept) fails in the frontend."""
    from can_distributed_pytorch_amd.ops import conv as CV
    ex = ctx.ex
    dispatch_cfg(ctx_linear=1)
    fv, dcat, _ = _inputs(n, h, w, ctx.dtype, seed=1000 * h + w)
    if w >= 64:
        cells = torch.zeros(n, 50, C, device="cuda")
        with pytest.raises(ValueError):
            CV.conv_ctx_fwd(fv, ex.ctx2cat_fwd, cells, cells)
        with pytest.raises(ValueError):
            CV.conv_ctx_bwd(torch.zeros(n, h, w, 4 * C, dtype=ctx.dtype, device="cuda"), ex.ctx2cat_dgr, cells, dcat,
                            fv)
    assert not ex._ctx_linear(fv)
    with pytest.raises(RuntimeError, match="rc=-7"):
        ex._context_fwd(fv, True)
    last = ex.front[-1]
    assert last.cout == C
    with pytest.raises(RuntimeError, match="rc=-7"):
        ex._conv(last, torch.zeros(n, h, w, last.cin, dtype=ctx.dtype, device="cuda"))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------- weight gradients
WGRAD_IDS = ["fresh", "accumulate", "accumulate-loss-scale", "accumulate-scale-eighth"]


def _wgrad_stages(cx, form, k, ops, fv, dcat, beta, scale, dscale):
    """The dW1 / dW2 stages: the executor's own _context_bwd (side=None: every launch on the compute stream) writes
    the eight conv{S}_1 / conv{S}_2 gradients into real buffers -- the dW2cat weight gradient, the scatter, the
    beta = 1 second term and the cell GEMMs of mode 2 as the schedule chains them -- and each is compared with
    ctx_reference.wgrad_stage of the kernels' own operands ``ops`` (teacher forcing: ``k`` holds the outputs of the
    fixed-order kernels, which the backward re-runs bitwise).  fv, dcat: the maps the executor is run on (padded in the
    padded case; ``ops`` then holds the valid columns).  The old contents are NaN at beta = 0 (not read) and random
    at the rms of the fresh gradient otherwise."""
    from can_distributed_pytorch_amd.ops import conv as CV
    ex = cx.ex
    arena = torch.full((8, C, C), float("nan"), dtype=torch.float32, device="cuda")
    g0 = None
    if beta != 0.0:
        gen = torch.Generator().manual_seed(17)
        fresh = R.wgrad_stage(form, ops, None, 0.0, 1.0, None)
        g0 = tuple(torch.randn(4, C, C, generator=gen).cuda() * f.pow(2).mean((1, 2), keepdim=True).sqrt().float()
                   for f in fresh)
        arena[:4], arena[4:] = g0
    grads = [None] * len(ex._params())
    for si, s in enumerate(SCALES):
        grads[ex.ctx1_index[s]] = arena[si].view(C, C, 1, 1)
        grads[ex.ctx2_index[s]] = arena[4 + si].view(C, C, 1, 1)
    dsc = None if dscale is None else torch.tensor([dscale], dtype=torch.float32, device="cuda")
    done = []
    ex._context_bwd(k["saved"], fv, dcat, grads, CV.WgradWorkspace(fv.device), beta, scale, done.extend, dsc, None)
    torch.cuda.synchronize()
    assert sorted(done) == sorted([ex.ctx1_index[s] for s in SCALES] + [ex.ctx2_index[s] for s in SCALES])
    ref1, ref2 = R.wgrad_stage(form, ops, g0, beta, scale, dscale)
    ck = Checks(cx, form)
    ck.wgrad32("dW1", arena[:4], ref1)
    ck.wgrad32("dW2", arena[4:], ref2)
    ck.done()


def _linear_ops(k, fv, w):
    """The operands of the linear form's weight gradients at the valid columns."""
    n, h = fv.shape[:2]
    return dict(fv=fv[:, :, :w], dg=_scales_first(k["dg"][:, :, :w], n, h, w), dt=k["dt"], u=k["u"],
                du_all=k["du_all"], ave=k["ave"])


@pytest.mark.parametrize("beta,scale,dscale", R.WGRAD_SETTINGS, ids=WGRAD_IDS)
@pytest.mark.parametrize("n,h,w", R.WGRAD_LINEAR_SHAPES)
def test_linear_wgrad_stages(ctx, dispatch_cfg, n, h, w, beta, scale, dscale):
    dispatch_cfg(ctx_linear=1)
    fv, dcat, dave_r = _inputs(n, h, w, ctx.dtype, seed=1000 * h + w)
    assert ctx.ex._ctx_linear(fv)
    k = _kernels_linear(ctx, fv, dcat, dave_r)
    _wgrad_stages(ctx, "linear", k, _linear_ops(k, fv, w), fv, dcat, beta, scale, dscale)


@pytest.mark.parametrize("beta,scale,dscale", R.WGRAD_SETTINGS, ids=WGRAD_IDS)
def test_linear_wgrad_stages_width_padded(ctx, dispatch_cfg, beta, scale, dscale):
    """The 127-column map at a row pitch of 128: the weight gradients are those of the 127-column map (the padding
    column of dG and fv is zero and adds nothing)."""
    n, h, w = R.PADDED_SHAPE
    pitch = 128
    dispatch_cfg(ctx_linear=1)
    fv, dcat, dave_r = _inputs(n, h, w, ctx.dtype, seed=1000 * h + w)
    fvp = torch.zeros(n, h, pitch, C, dtype=ctx.dtype, device="cuda")
    fvp[:, :, :w] = fv
    dcatp = torch.zeros(n, h, pitch, 2 * C, dtype=ctx.dtype, device="cuda")
    dcatp[:, :, :w] = dcat
    k = _kernels_linear(ctx, fvp, dcatp, dave_r, wv=w)
    assert k["saved"]["wv"] == w
    _wgrad_stages(ctx, "linear", k, _linear_ops(k, fvp, w), fvp, dcatp, beta, scale, dscale)


@pytest.mark.parametrize("beta,scale,dscale", R.WGRAD_SETTINGS, ids=WGRAD_IDS)
@pytest.mark.parametrize("n,h,w", R.WGRAD_DIRECT_SHAPES)
def test_direct_wgrad_stages(ctx, dispatch_cfg, n, h, w, beta, scale, dscale):
    fv, dcat, dave_r = _inputs(n, h, w, ctx.dtype, seed=1000 * h + w)
    assert not ctx.ex._ctx_linear(fv)
    k = _kernels_direct(ctx, fv, dcat, dave_r)
    ops = dict(dz=k["dz"], cs=k["cs"], dA=k["dA"], ave=k["ave"])
    _wgrad_stages(ctx, "direct", k, ops, fv, dcat, beta, scale, dscale)


# ------------------------------------------------------------------------------------------------------ batch isolation
@pytest.mark.parametrize("linear,n,h,w", [(True, 3, 5, 65), (False, 3, 2, 3)])
def test_batch_isolation_bitwise(ctx, dispatch_cfg, linear, n, h, w):
    """Another image in the middle of the batch leaves every output of images 0 and 2 bitwise unchanged (the
    kernels sum in a fixed order): no kernel reads a neighbour's cell table or pixels."""
    dispatch_cfg(ctx_linear=1)
    fv, dcat, dave_r = _inputs(n, h, w, ctx.dtype, seed=77)
    run = _kernels_linear if linear else _kernels_direct
    a = run(ctx, fv, dcat, dave_r)
    fv2 = fv.clone()
    fv2[1] = R.structured_fv(1, h, w, C, ctx.dtype, seed=78, device="cuda")[0]
    assert not torch.equal(fv2[1], fv[1])
    b = run(ctx, fv2, dcat, dave_r)
    names = ("ave", "wts", "cat", "dt", "du", "dfv") if linear else ("ave", "wts", "cat", "dA", "dfv")
    for name in names:
        x, y = a[name], b[name]
        if name == "wts" and not linear:               # [4, N, h, w, C]
            x, y = x.transpose(0, 1), y.transpose(0, 1)
        assert torch.equal(x[0], y[0]) and torch.equal(x[2], y[2]), f"{name} of images 0 / 2 changed"
        assert not torch.equal(x[1], y[1]), f"{name} of image 1 did not change"
