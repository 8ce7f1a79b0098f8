"""The staged fp64 reference of the context module (tests/ctx_reference.py), checked on the CPU:

* its pooling / upsampling matrices against ATen in fp64, at every length the kernels treat differently;
* its composed forward against the reference math of tests/test_gpu_context.py::_ref_context and every backward
  piece against fp64 autograd;
* the kernels' two-bin assumption of the pooling adjoint (conv_igemm.hip ctx_pool_cols) against the true bins;
* the sensitivity of the stage checks of tests/test_gpu_context_stages.py: on the structured inputs and at the shapes
  of that test, the clean reference rounded to bf16 / fp16 passes every stage check with zero outliers, and every
  deliberate mistake in the reference's OWN geometry fails the check of the stage that owns it, forward and adjoint
  (the pattern of tests/test_numerics_checker.py).  No project code is perturbed and nothing here runs on a GPU;
* the cell GEMM references (forward, transpose, weight gradient over cells) against fp64 matmuls and autograd, and the
  sensitivity of the dW1 / dW2 stage checks to every mistake of ctx_reference.WGRAD_MISTAKES.
"""
import types

import pytest
import torch
import torch.nn.functional as F

import ctx_reference as R
from ctx_reference import F64, SCALES

LENGTHS = list(range(1, 21)) + [45, 64, 65, 67, 96, 127, 128]


# ---------------------------------------------------------------------------------------------- matrices against ATen
@pytest.mark.parametrize("S", SCALES)
def test_matrices_vs_aten(S):
    for L in LENGTHS:
        pool = F.adaptive_avg_pool2d(torch.eye(L, dtype=F64).view(L, 1, L, 1), (S, 1)).view(L, S).t()
        assert (R.pool_matrix(S, L) - pool).abs().max().item() <= 1e-12, ("pool", S, L)
        up = F.interpolate(torch.eye(S, dtype=F64).view(S, 1, S, 1), size=(L, 1), mode="bilinear",
                           align_corners=True).view(S, L).t()
        assert (R.bilinear_matrix(S, L) - up).abs().max().item() <= 1e-12, ("bilinear", S, L)


def test_cell_layout_round_trip():
    cells = torch.arange(2 * 50 * 3, dtype=F64).view(2, 50, 3)
    grids = R.cells_to_grids(cells)
    assert [tuple(g.shape) for g in grids] == [(2, 3, S, S) for S in SCALES]
    assert grids[3][1, 2, 4, 5].item() == cells[1, 14 + 4 * 6 + 5, 2].item()
    assert torch.equal(R.grids_to_cells(grids), cells)


def test_pool_bins_overlap_at_most_two_from_length_3():
    """The EPI_CTXB epilogue's pooling adjoint adds at most two row bins per scale at a pixel (conv_igemm.hip
    ctx_pool_cols: the bin floor(x S / L) and one neighbour).  That holds from L = 3 on; at L = 1 and 2 the bins of
    the 3- and 6-grids repeat and a pixel lies in up to 6 of them, which is why ops.conv.ctx_linear_ok sends maps of
    fewer than 3 rows to the direct form (context.hip ctx_bwd_final loops over every bin)."""
    for S in SCALES:
        for L in LENGTHS:
            m = R.pool_matrix(S, L)
            per_pixel = int((m > 0).sum(0).max())
            if L >= 3:
                assert per_pixel <= 2, (S, L, per_pixel)
                for x in range(L):                       # and they are ctx_pool_cols' two
                    jA = (x * S) // L
                    got = {jA}
                    if jA > 0 and -((-jA * L) // S) > x:
                        got.add(jA - 1)
                    elif jA + 1 < S and ((jA + 1) * L) // S <= x:
                        got.add(jA + 1)
                    assert got == set(torch.nonzero(m[:, x]).flatten().tolist()), (S, L, x)
    assert int((R.pool_matrix(6, 1) > 0).sum(0).max()) == 6 and int((R.pool_matrix(6, 2) > 0).sum(0).max()) == 3
    assert int((R.pool_matrix(3, 1) > 0).sum(0).max()) == 3


# -------------------------------------------------------------------------- composed stages against ATen and autograd
def _weights(c, seed, std):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(4, c, c, generator=g, dtype=F64) * std, torch.randn(4, c, c, generator=g, dtype=F64) * std)


def _close(a, b, what):
    err = (a - b).abs().max().item()
    assert err <= 1e-10 * max(1.0, b.abs().max().item()), (what, err)


@pytest.mark.parametrize("n,h,w", [(2, 5, 7), (1, 1, 9), (2, 13, 4), (1, 6, 12)])
def test_composed_stages_vs_aten_fp64(n, h, w):
    from test_gpu_context import _ref_context
    c = 8
    W1, W2 = _weights(c, 3, 0.4)
    model = types.SimpleNamespace()
    for si, S in enumerate(SCALES):
        for k, W in ((1, W1), (2, W2)):
            conv = torch.nn.Conv2d(c, c, 1, bias=False).double()
            with torch.no_grad():
                conv.weight.copy_(W[si].view(c, c, 1, 1))
            setattr(model, f"conv{S}_{k}", conv)
    geo = R.Geometry(h, w)
    fv = R.structured_fv(n, h, w, c, torch.bfloat16, seed=5).double()
    fr = fv.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    cr = _ref_context(model, fr)
    fi_ref = cr[:, c:].permute(0, 2, 3, 1)
    _close(R.context_forward(fv, W1, W2, geo, linear=True), fi_ref.detach(), "fi, linear form")
    _close(R.context_forward(fv, W1, W2, geo, linear=False), fi_ref.detach(), "fi, direct form")
    # the whole backward, both forms
    g = torch.Generator().manual_seed(9)
    dcat = torch.randn(n, h, w, 2 * c, generator=g, dtype=F64)
    (dfr,) = torch.autograd.grad(cr, fr, dcat.permute(0, 3, 1, 2))
    dfv_ref = (dfr * (fr > 0)).permute(0, 2, 3, 1)
    _close(R.context_backward(fv, dcat, W1, W2, geo, linear=True), dfv_ref, "dfv, linear form")
    _close(R.context_backward(fv, dcat, W1, W2, geo, linear=False), dfv_ref, "dfv, direct form")

    # the pieces, each against autograd of the ATen op it transposes
    def nchw(t):
        return t.permute(0, 3, 1, 2)
    fl = fv.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    pooled = [F.adaptive_avg_pool2d(fl, (S, S)) for S in SCALES]
    _close(R.pool_cells(fv, geo), R.grids_to_cells([p.detach() for p in pooled]), "pool_cells")
    dave = torch.randn(n, 50, c, generator=g, dtype=F64)
    (dp,) = torch.autograd.grad(pooled, fl, R.cells_to_grids(dave))
    _close(R.pool_adjoint(dave, geo), dp.permute(0, 2, 3, 1), "pool_adjoint")
    cells = torch.randn(n, 50, c, generator=g, dtype=F64)
    grids = [gr.contiguous().requires_grad_(True) for gr in R.cells_to_grids(cells)]
    ups = [F.interpolate(gr, size=(h, w), mode="bilinear", align_corners=True) for gr in grids]
    s = R.upsample(cells, geo)
    _close(s, torch.stack([u.detach().permute(0, 2, 3, 1) for u in ups]), "upsample")
    maps = torch.randn(4, n, h, w, c, generator=g, dtype=F64)
    dgr = torch.autograd.grad(ups, grids, [nchw(m) for m in maps])
    _close(R.upsample_adjoint(maps, geo), R.grids_to_cells(list(dgr)), "upsample_adjoint")
    _close(R.direct_c(cells, fv, geo), s - fv[None], "direct_c")
    # dz / ds (= sdir): gradients of fi with respect to z and s as independent leaves
    z = torch.randn(4, n, h, w, c, generator=g, dtype=F64).requires_grad_(True)
    sl = s.clone().requires_grad_(True)
    wts = torch.sigmoid(z)
    fi = (wts * sl).sum(0) / (wts.sum(0) + 1e-12)
    dfi = dcat[..., c:]
    dz_ref, ds_ref = torch.autograd.grad(fi, [z, sl], dfi)
    dz, ds = R.bwd_pointwise(dfi, wts.detach(), s)
    _close(dz, dz_ref, "dz")
    _close(ds, ds_ref, "ds / sdir")
    _close(R.fuse(wts.detach(), s), fi.detach(), "fuse")


# ------------------------------------------------------------------------------------------------------- sensitivity
def _late_start(geo, n):
    """The last column bin of scale 6 starts one pixel late."""
    st, en = R.pool_bins(6, geo.w)[-1]
    if en - st < 2:
        return None
    g = geo.clone()
    g.Px[3][5] = 0
    g.Px[3][5, st + 1:en] = 1.0 / (en - st - 1)
    return g


def _divisor(geo, n):
    """The last column bin's divisor counts one padding column."""
    st, en = R.pool_bins(6, geo.w)[-1]
    g = geo.clone()
    g.Px[3][5] *= (en - st) / (en - st + 1.0)
    return g


def _segment_column(geo, n):
    """One column at a row-segment boundary (x = w / 4) is missing from every pooled sum."""
    g = geo.clone()
    for si in range(4):
        g.Px[si][:, geo.w // 4] = 0
    return g


def _last_column(geo, n):
    """The upsample's last column repeats the one before."""
    if geo.w < 2:
        return None
    g = geo.clone()
    for si in range(4):
        g.Bx[si][geo.w - 1] = g.Bx[si][geo.w - 2]
    return g


def _roll(geo, n):
    """Every cell table belongs to the next image of the batch."""
    if n < 2:
        return None
    g = geo.clone()
    g.cell_read = g.cell_write = lambda cells: cells.roll(1, 0)
    return g


def _swap(geo, n):
    """i and j swapped inside the cells of scales 3 and 6."""
    def swap(cells):
        grids = R.cells_to_grids(cells)
        return R.grids_to_cells(grids[:2] + [gr.transpose(2, 3) for gr in grids[2:]])
    g = geo.clone()
    g.cell_read = g.cell_write = swap
    return g


POOL_MUTATIONS = [_late_start, _divisor, _segment_column, _roll, _swap]      # owned by the pooling stage
UP_MUTATIONS = [_last_column, _roll, _swap]                                  # owned by the upsampling stage
MUTATIONS = list(dict.fromkeys(POOL_MUTATIONS + UP_MUTATIONS))
STAGE_SHAPES = R.LINEAR_SHAPES + [R.PADDED_SHAPE] + R.DIRECT_SHAPES
C_CPU = 32            # channels here; the weights' std keeps the magnitudes of the 512-channel module (std 0.05)
W_STD = 0.05 * (512 / C_CPU) ** 0.5


def _stage_outputs(geo, fv, dcat, dave, W1, W2):
    """Every quantity the GPU stage checks compare, from the reference under ``geo``; each stage from the CLEAN
    upstream values (teacher forcing), so a wrong geometry shows only in the stages that use the wrong matrix."""
    clean = R.Geometry(geo.h, geo.w)
    c = fv.shape[3]
    ave = R.pool_cells(fv, clean)
    u = R.conv1x1_cells(ave, W1)
    t = R.conv1x1_cells(u, W2)
    wts, _, s = R.weights_and_fi(fv, u, t, W2, clean)
    dz, ds = R.bwd_pointwise(dcat[..., c:], wts, s)
    mask = fv.to(F64) > 0
    out = dict(ave=R.pool_cells(fv, geo), pool_adj=R.pool_adjoint(dave, geo) * mask, c=R.direct_c(u, fv, geo),
               dt=R.upsample_adjoint(dz, geo), du=R.upsample_adjoint(ds, geo))
    out["w"], out["fi"], _ = R.weights_and_fi(fv, u, t, W2, geo)
    out["dz"], out["ds"] = R.bwd_pointwise(dcat[..., c:], wts, R.upsample(u, geo))
    return out


def _ratios(got, ref, fv, geo):
    """err / bound of every stage check: the pooled cells' own bound, check_out16 for the 16-bit maps, check_sum32
    (scale by scale) for the fp32 cell tables."""
    r = {k: R.out16_ratio(got[k], ref[k]) for k in ("pool_adj", "c", "w", "fi", "dz", "ds")}
    r["ave"] = R.pool_ratio(got["ave"], fv, geo, ref=ref["ave"])
    r["dt"] = R.cells_sum32_ratio(got["dt"], ref["dt"])
    r["du"] = R.cells_sum32_ratio(got["du"], ref["du"])
    return r


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n,h,w", STAGE_SHAPES)
def test_stage_checks_pass_clean_and_catch_every_mutation(n, h, w, dtype):
    geo = R.Geometry(h, w)
    W1, W2 = _weights(C_CPU, 11, W_STD)
    W2 = W2.to(dtype).to(F64)
    fv = R.structured_fv(n, h, w, C_CPU, dtype, seed=100 * h + w)
    g = torch.Generator().manual_seed(7)
    dcat = torch.randn(n, h, w, 2 * C_CPU, generator=g).to(dtype)
    dave = torch.randn(n, 50, C_CPU, generator=g)
    ref = _stage_outputs(geo, fv, dcat, dave, W1, W2)
    # what a correct kernel returns: the reference rounded to the stage's storage type
    got = {k: (v.float() if k in ("ave", "dt", "du") else v.to(dtype)) for k, v in ref.items()}
    clean = _ratios(got, ref, fv, geo)
    assert all(v <= 1.0 for v in clean.values()), clean
    live = 0
    for mut in MUTATIONS:
        bad_geo = mut(geo, n)
        if bad_geo is None:                 # the mistake cannot be made at this shape (one image, one column, ...)
            continue
        live += 1
        r = _ratios(got, _stage_outputs(bad_geo, fv, dcat, dave, W1, W2), fv, geo)
        if mut in POOL_MUTATIONS:
            assert r["ave"] > 1.0 and r["pool_adj"] > 1.0, (mut.__name__, "pooling stage", r)
        if mut in UP_MUTATIONS:
            assert r["c"] > 1.0 and r["fi"] > 1.0, (mut.__name__, "upsampling stage, forward", r)
            assert r["dt"] > 1.0 and r["du"] > 1.0, (mut.__name__, "upsampling stage, adjoint", r)
    assert live >= 3, live


# ------------------------------------------------------------------------------------- cell GEMMs and weight gradients
@pytest.mark.parametrize("n,c", [(1, 8), (3, 16)])
def test_cell_gemms_vs_torch_fp64(n, c):
    """conv1x1_cells, its transpose and the per-scale weight gradient over cells (the three modes of the kernels'
    ctx_gemm) against plain fp64 matmuls on the [N, 50, C] layout, scale by scale; wgrad_maps against autograd."""
    g = torch.Generator().manual_seed(21 + n)
    x = torch.randn(n, 50, c, generator=g, dtype=F64)
    d = torch.randn(n, 50, c, generator=g, dtype=F64)
    W = torch.randn(4, c, c, generator=g, dtype=F64)
    fwd, bwd, dw = R.conv1x1_cells(x, W), R.conv1x1_cells_t(d, W), R.wgrad_cells(d, x)
    assert fwd.shape == bwd.shape == (n, 50, c) and dw.shape == (4, c, c)
    for si, (S, o) in enumerate(zip(SCALES, R.CELL_OFF)):
        rows_x, rows_d = x[:, o:o + S * S].reshape(-1, c), d[:, o:o + S * S].reshape(-1, c)
        _close(fwd[:, o:o + S * S].reshape(-1, c), rows_x @ W[si].t(), ("forward", S))
        _close(bwd[:, o:o + S * S].reshape(-1, c), rows_d @ W[si], ("transpose", S))
        _close(dw[si], rows_d.t() @ rows_x, ("weight gradient", S))
    # and as gradients of <d, conv1x1_cells(x, W)> by autograd
    xl, Wl = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    gx, gW = torch.autograd.grad((R.conv1x1_cells(xl, Wl) * d).sum(), [xl, Wl])
    _close(bwd, gx, "transpose, autograd")
    _close(dw, gW, "weight gradient, autograd")
    maps = torch.randn(4, n, 3, 5, c, generator=g, dtype=F64)
    dm = torch.randn(4, n, 3, 5, c, generator=g, dtype=F64)
    Wm = W.clone().requires_grad_(True)
    (gm,) = torch.autograd.grad((R.conv1x1_maps(maps, Wm) * dm).sum(), [Wm])
    _close(R.wgrad_maps(dm, maps), gm, "wgrad_maps")
    (g1,) = torch.autograd.grad((R.conv1x1_maps(maps[0][None].expand(4, -1, -1, -1, -1), Wm) * dm).sum(), [Wm])
    _close(R.wgrad_maps(dm, maps[0]), g1, "wgrad_maps, one input")


def _wgrad_operands(form, n, h, w, dtype, std=W_STD):
    """The operands of the weight-gradient stages as correct kernels would hold them (16-bit maps, fp32 cells), from
    the clean reference at C_CPU channels."""
    geo = R.Geometry(h, w)
    W1, W2 = _weights(C_CPU, 11, std)
    W2 = W2.to(dtype).to(F64)
    fv = R.structured_fv(n, h, w, C_CPU, dtype, seed=100 * h + w)
    g = torch.Generator().manual_seed(7)
    dfi = torch.randn(n, h, w, 2 * C_CPU, generator=g).to(dtype)[..., C_CPU:]
    ave = R.pool_cells(fv, geo).float()
    u = R.conv1x1_cells(ave, W1).float()
    s = R.upsample(u, geo)
    if form == "linear":
        wts = R.weights_and_fi(fv, u, R.conv1x1_cells(u, W2), W2, geo)[0].to(dtype)
        dz, ds = R.bwd_pointwise(dfi, wts, s)
        dt = R.upsample_adjoint(dz, geo).float()
        du_all = (R.upsample_adjoint(ds, geo) + R.conv1x1_cells_t(dt, W2)).float()
        return dict(fv=fv, dg=(-dz).to(dtype), dt=dt, u=u, du_all=du_all, ave=ave)
    cs = R.direct_c(u, fv, geo).to(dtype)
    wts = torch.sigmoid(R.conv1x1_maps(cs, W2)).to(dtype)
    dz, sdir = R.bwd_pointwise(dfi, wts, s)
    dz = dz.to(dtype)
    dc = R.conv1x1_maps(dz, W2.transpose(1, 2)).to(dtype)
    dA = R.upsample_adjoint(sdir.to(dtype).to(F64) + dc.to(F64), geo).float()
    return dict(dz=dz, cs=cs, dA=dA, ave=ave)


WGRAD_CASES = [("linear",) + s for s in R.WGRAD_LINEAR_SHAPES + [R.PADDED_SHAPE]] + \
              [("direct",) + s for s in R.WGRAD_DIRECT_SHAPES]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("form,n,h,w", WGRAD_CASES)
def test_wgrad_stage_checks_pass_clean_and_catch_every_mistake(form, n, h, w, dtype):
    """The dW1 / dW2 stage checks of tests/test_gpu_context_stages.py (check_sum32 at its default 1e-3, scale by
    scale) on the CPU, at the same shapes and (beta, scale, dscale) settings with C_CPU channels: the reference
    rounded to fp32 passes, and every mistake of ctx_reference.WGRAD_MISTAKES pushes at least one scale of every
    gradient that owns it over the bound, wherever it can be made.  The conv{S}_1 / conv{S}_2 std is the module
    tests' 0.05 (W_STD at C_CPU channels): dt^T u is large enough to be seen at it, so it is not raised."""
    k = _wgrad_operands(form, n, h, w, dtype)
    gen = torch.Generator().manual_seed(13)
    seen = set()
    for beta, scale, dscale in R.WGRAD_SETTINGS:
        fresh = R.wgrad_stage(form, k, None, 0.0, 1.0, None)
        # old contents at the rms of the fresh gradient, as the GPU test draws them
        g0 = tuple(torch.randn(f.shape, generator=gen) * f.pow(2).mean((1, 2), keepdim=True).sqrt().float()
                   for f in fresh)
        ref = dict(zip(("dW1", "dW2"), R.wgrad_stage(form, k, g0, beta, scale, dscale)))
        for name, r in ref.items():
            assert R.wgrad_sum32_ratio(r.float(), r) <= 1.0, (name, "clean")
        for mistake, owners in R.WGRAD_MISTAKES.items():
            if not R.wgrad_mistake_live(mistake, form, n, beta, scale, dscale):
                continue
            seen.add(mistake)
            bad = dict(zip(("dW1", "dW2"), R.wgrad_stage(form, k, g0, beta, scale, dscale, mistake)))
            for name in ("dW1", "dW2"):
                ratio = R.wgrad_sum32_ratio(ref[name].float(), bad[name])
                if name in owners[form]:
                    assert ratio > 1.0, (mistake, name, (beta, scale, dscale), ratio)
                else:
                    assert ratio <= 1.0, (mistake, name, "a gradient the mistake does not touch", ratio)
    assert seen == {m for m, o in R.WGRAD_MISTAKES.items() if form in o}, seen


def test_every_mutation_is_live_at_some_shape():
    for mut in MUTATIONS:
        assert sum(mut(R.Geometry(h, w), n) is not None for n, h, w in STAGE_SHAPES) >= 6, mut.__name__
