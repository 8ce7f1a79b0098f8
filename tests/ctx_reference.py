"""Staged fp64 reference of the multi-scale context module (model/CANNet.py:42-87; csrc/context.hip, the EPI_CTXF /
EPI_CTXB epilogues of csrc/conv_igemm.hip).

Every geometric step of the module is linear, and here each one is an explicit matrix built in Python from its
definition (no ATen call): adaptive average pooling to the 1/2/3/6 grids (``pool_matrix``), the ``align_corners``
bilinear upsample of the cell tables (``bilinear_matrix``) and, by transposition, the adjoints of both.  A ``Geometry``
holds the matrices of one map size; the stage functions take it as an argument, so a test can hand them a deliberately
wrong geometry (tests/test_ctx_reference_cpu.py) and see which check notices.

Layouts are the kernels': maps [N, h, w, C], the stack of the four scales' maps [4, N, h, w, C], cell tables
[N, 50, C] with the S x S cells of scale S at offset 0 / 1 / 5 / 14 (cell (i, j) at offset + i * S + j), the four
1x1 conv weights [4, C_out, C_in].  Everything is computed in fp64 on the device of its inputs.
"""
import math

import torch

from numerics import ATOL16_RMS, RTOL16

SCALES = (1, 2, 3, 6)
CELL_OFF = (0, 1, 5, 14)
NCELL = 50
F64 = torch.float64

# (n, h, w) of the stage tests: the smallest maps at which each mechanism of the kernels is exercised.  Linear form
# (w >= 64): one row; lengths that are no multiple of 4 (the row pass's column segments) with fewer than 9 rows; h < 6
# and h = 6, 7 around the 6-grid; several 256-pixel GEMM tiles.  Direct form: lengths below the 6-grid in either
# direction, odd sizes, the map of a 384 x 384 crop, and a wide map with the linear form switched off.
LINEAR_SHAPES = [(1, 1, 64), (3, 5, 65), (2, 6, 67), (1, 7, 70), (2, 13, 96), (1, 17, 127)]
PADDED_SHAPE = (2, 12, 127)          # run as a padded map of pitch 128
DIRECT_SHAPES = [(1, 1, 5), (2, 5, 1), (3, 2, 3), (1, 6, 7), (2, 13, 17), (1, 48, 48), (1, 12, 128)]


# ---------------------------------------------------------------------------------------------------------- matrices
def pool_bins(S, L):
    """ATen's adaptive-pool bins over a length L: [floor(i L / S), ceil((i + 1) L / S)), overlapping when L % S != 0
    and repeating when L < S."""
    return [((i * L) // S, -((-(i + 1) * L) // S)) for i in range(S)]


def pool_matrix(S, L):
    """[S, L]: row i averages bin i."""
    m = torch.zeros(S, L, dtype=F64)
    for i, (st, en) in enumerate(pool_bins(S, L)):
        m[i, st:en] = 1.0 / (en - st)
    return m


def bilinear_matrix(S, L):
    """[L, S]: bilinear upsample of S cells to L positions, align_corners=True."""
    m = torch.zeros(L, S, dtype=F64)
    scale = (S - 1) / (L - 1) if L > 1 else 0.0
    for x in range(L):
        src = scale * x
        x0 = min(int(math.floor(src)), S - 1)
        x1 = min(x0 + 1, S - 1)
        lam = src - x0
        m[x, x0] += 1.0 - lam
        m[x, x1] += lam
    return m


class Geometry:
    """The pooling (Py [S, h], Px [S, w]) and upsampling (By [h, S], Bx [w, S]) matrices of an h x w map, per scale.
    ``cell_read`` / ``cell_write`` (None: identity) are applied to every cell table a stage reads / writes: the hooks
    by which the sensitivity test misplaces cells."""

    def __init__(self, h, w, device="cpu"):
        self.h, self.w = h, w
        self.Py = [pool_matrix(S, h).to(device) for S in SCALES]
        self.Px = [pool_matrix(S, w).to(device) for S in SCALES]
        self.By = [bilinear_matrix(S, h).to(device) for S in SCALES]
        self.Bx = [bilinear_matrix(S, w).to(device) for S in SCALES]
        self.cell_read = None
        self.cell_write = None

    def clone(self):
        g = Geometry.__new__(Geometry)
        g.h, g.w = self.h, self.w
        for k in ("Py", "Px", "By", "Bx"):
            setattr(g, k, [m.clone() for m in getattr(self, k)])
        g.cell_read, g.cell_write = self.cell_read, self.cell_write
        return g

    def _read(self, cells):
        return cells if self.cell_read is None else self.cell_read(cells)

    def _write(self, cells):
        return cells if self.cell_write is None else self.cell_write(cells)


# -------------------------------------------------------------------------------------------------------- cell layout
def cells_to_grids(cells):
    """[N, 50, C] -> the four grids [N, C, S, S]."""
    n, _, c = cells.shape
    return [cells[:, o:o + S * S].reshape(n, S, S, c).permute(0, 3, 1, 2) for S, o in zip(SCALES, CELL_OFF)]


def grids_to_cells(grids):
    """The four grids [N, C, S, S] -> [N, 50, C]."""
    n, c = grids[0].shape[:2]
    return torch.cat([g.permute(0, 2, 3, 1).reshape(n, -1, c) for g in grids], 1)


def _grid(cells, si):
    """Scale si's cells as [N, S, S, C]."""
    S, o = SCALES[si], CELL_OFF[si]
    return cells[:, o:o + S * S].reshape(cells.shape[0], S, S, cells.shape[2])


def cell_pixels(geo, device="cpu"):
    """[50]: pixel count K of each pooled cell's bin."""
    out = []
    for S in SCALES:
        ky = torch.tensor([en - st for st, en in pool_bins(S, geo.h)], dtype=F64)
        kx = torch.tensor([en - st for st, en in pool_bins(S, geo.w)], dtype=F64)
        out.append((ky[:, None] * kx[None, :]).reshape(-1))
    return torch.cat(out).to(device)


# ------------------------------------------------------------------------------------------------------------ forward
def pool_cells(fv, geo):
    """fv [N, h, w, C] -> ave [N, 50, C]."""
    x = fv.to(F64)
    n, c = x.shape[0], x.shape[3]
    cells = [torch.einsum("iy,nyxc,jx->nijc", geo.Py[si], x, geo.Px[si]).reshape(n, -1, c) for si in range(4)]
    return geo._write(torch.cat(cells, 1))


def upsample(cells, geo):
    """cells [N, 50, C] -> [4, N, h, w, C]."""
    t = geo._read(cells.to(F64))
    return torch.stack([torch.einsum("yi,nijc,xj->nyxc", geo.By[si], _grid(t, si), geo.Bx[si]) for si in range(4)])


def conv1x1_cells(cells, W):
    """The 1x1 conv of scale S on its own cells: cells [N, 50, C], W [4, C_out, C_in] -> [N, 50, C_out]."""
    t, Wd = cells.to(F64), W.to(F64)
    return torch.cat([_grid(t, si).reshape(t.shape[0], -1, t.shape[2]) @ Wd[si].t() for si in range(4)], 1)


def conv1x1_cells_t(cells, W):
    """The transposed 1x1 conv (its data gradient): cells [N, 50, C_out], W [4, C_out, C_in] -> [N, 50, C_in]."""
    t, Wd = cells.to(F64), W.to(F64)
    return torch.cat([_grid(t, si).reshape(t.shape[0], -1, t.shape[2]) @ Wd[si] for si in range(4)], 1)


def wgrad_cells(d, x):
    """The 1x1 convs' weight gradients over the cells: d [N, 50, C_out], x [N, 50, C_in] -> [4, C_out, C_in],
    dW_S = sum over the N S^2 cells of scale S of d[cell] x[cell]^T."""
    dd, xd = d.to(F64), x.to(F64)
    return torch.stack([torch.einsum("nrc,nrk->ck", dd[:, o:o + S * S], xd[:, o:o + S * S])
                        for S, o in zip(SCALES, CELL_OFF)])


def wgrad_maps(d, x):
    """The 1x1 convs' weight gradients over maps: d [4, N, h, w, C_out], x [4, N, h, w, C_in] or [N, h, w, C_in] (one
    input for the four scales) -> [4, C_out, C_in]."""
    dd, xd = d.to(F64), x.to(F64)
    return torch.einsum("snyxc,snyxk->sck" if xd.dim() == 5 else "snyxc,nyxk->sck", dd, xd)


def conv1x1_maps(maps, W):
    """maps [4, N, h, w, C_in], W [4, C_out, C_in] -> [4, N, h, w, C_out] (scale S's conv on scale S's map)."""
    return torch.einsum("snyxk,sck->snyxc", maps.to(F64), W.to(F64))


def fuse(wts, s):
    """fi = sum_S w_S s_S / (sum_S w_S + 1e-12); wts, s [4, N, h, w, C]."""
    wd, sd = wts.to(F64), s.to(F64)
    return (wd * sd).sum(0) / (wd.sum(0) + 1e-12)


def weights_and_fi(fv, u, t, W2, geo):
    """The linearised form: z_S = up(t_S) - W2_S fv, w_S = sigmoid(z_S), fi = fuse(w, up(u)).  -> (w, fi, s)."""
    x = fv.to(F64)
    g = torch.einsum("nyxk,sck->snyxc", x, W2.to(F64))
    wts = torch.sigmoid(upsample(t, geo) - g)
    s = upsample(u, geo)
    return wts, fuse(wts, s), s


def direct_c(table, fv, geo):
    """The direct form's c_S = up(A_S) - fv, [4, N, h, w, C]."""
    return upsample(table, geo) - fv.to(F64)[None]


def context_forward(fv, W1, W2, geo, linear=True, store=None, stored_w=None, parts=False):
    """The whole module in fp64 from fv [N, h, w, C] and the conv{S}_1 / conv{S}_2 weights [4, C, C] -> fi
    (parts: -> (w, fi)).
    store (a 16-bit dtype): the direct form's two storage points are followed, the c_S maps and the sigmoid maps
    rounded to it (the kernels keep both as 16-bit buffers: ctx_expand writes c_S for the conv{S}_2 GEMMs, whose
    sigmoid epilogue writes w for ctx_fuse); stored_w [4, N, h, w, C]: fi is formed from these w instead (a kernel's
    own buffer).  The linear form has no such point: its epilogue forms fi from the fp32 w."""
    u = conv1x1_cells(pool_cells(fv, geo), W1)
    if linear:
        wts, fi, _ = weights_and_fi(fv, u, conv1x1_cells(u, W2), W2, geo)
        return (wts, fi) if parts else fi
    c = direct_c(u, fv, geo)
    wts = torch.sigmoid(conv1x1_maps(c if store is None else c.to(store), W2))
    if stored_w is not None:
        wts = stored_w
    elif store is not None:
        wts = wts.to(store)
    fi = fuse(wts, upsample(u, geo))
    return (wts, fi) if parts else fi


# ----------------------------------------------------------------------------------------------------------- backward
def bwd_pointwise(dfi, wts, s):
    """g = dfi / D, D = sum_S w_S + 1e-12: dz_S = g (s_S - fi) w_S (1 - w_S) and ds_S = g w_S (the linear form's ds,
    the direct form's sdir), each [4, N, h, w, C], from the saved w and the upsampled table s."""
    wd, sd = wts.to(F64), s.to(F64)
    den = wd.sum(0) + 1e-12
    fi = (wd * sd).sum(0) / den
    g = dfi.to(F64) / den
    return g * (sd - fi) * wd * (1.0 - wd), g * wd


def upsample_adjoint(maps, geo):
    """maps [4, N, h, w, C] -> cells [N, 50, C]: the transposed upsample."""
    m = maps.to(F64)
    n, c = m.shape[1], m.shape[4]
    cells = [torch.einsum("yi,nyxc,xj->nijc", geo.By[si], m[si], geo.Bx[si]).reshape(n, -1, c) for si in range(4)]
    return geo._write(torch.cat(cells, 1))


def pool_adjoint(dave, geo):
    """dave [N, 50, C] -> [N, h, w, C]: the transposed pooling, summed over the four scales."""
    d = geo._read(dave.to(F64))
    return sum(torch.einsum("iy,nijc,jx->nyxc", geo.Py[si], _grid(d, si), geo.Px[si]) for si in range(4))


def dfv_linear(dg, W2, dcat_fv, dave, fv, geo):
    """(dG . W2cat + dcat[..., :C] + pool^T(dave)) (fv > 0) with dG [4, N, h, w, C] = -dz."""
    back = torch.einsum("snyxc,sck->nyxk", dg.to(F64), W2.to(F64))
    return (back + dcat_fv.to(F64) + pool_adjoint(dave, geo)) * (fv.to(F64) > 0)


def dfv_direct(dc, dcat_fv, dave, fv, geo):
    """(dcat[..., :C] - sum_S dc_S + pool^T(dave)) (fv > 0) with dc [4, N, h, w, C]."""
    return (dcat_fv.to(F64) - dc.to(F64).sum(0) + pool_adjoint(dave, geo)) * (fv.to(F64) > 0)


def context_backward(fv, dcat, W1, W2, geo, linear=True):
    """The whole backward in fp64, composed from the pieces above -> dfv [N, h, w, C] (ReLU mask applied)."""
    c = fv.shape[3]
    ave = pool_cells(fv, geo)
    u = conv1x1_cells(ave, W1)
    W1t, W2t = W1.to(F64).transpose(1, 2), W2.to(F64).transpose(1, 2)
    dfi, dcat_fv = dcat[..., c:], dcat[..., :c]
    if linear:
        wts, _, s = weights_and_fi(fv, u, conv1x1_cells(u, W2), W2, geo)
        dz, ds = bwd_pointwise(dfi, wts, s)
        dt = upsample_adjoint(dz, geo)
        du = upsample_adjoint(ds, geo) + conv1x1_cells(dt, W2t)
        return dfv_linear(-dz, W2, dcat_fv, conv1x1_cells(du, W1t), fv, geo)
    s = upsample(u, geo)
    wts = torch.sigmoid(conv1x1_maps(s - fv.to(F64)[None], W2))
    dz, sdir = bwd_pointwise(dfi, wts, s)
    dc = conv1x1_maps(dz, W2t)
    dA = upsample_adjoint(sdir + dc, geo)
    return dfv_direct(dc, dcat_fv, conv1x1_cells(dA, W1t), fv, geo)


# --------------------------------------------------------------------------------------------------- weight gradients
# (n, h, w) of the weight-gradient stages (a subset of the shapes above; PADDED_SHAPE joins the linear ones) and their
# (beta, scale, dscale) settings: a fresh gradient, the accumulation window, the fp16 step's loss scale on top of it.
# In the third, scale * dscale = 1: a term that misses the whole factor cannot be told there, hence the fourth (1 / 8)
WGRAD_LINEAR_SHAPES = [(3, 5, 65), (2, 13, 96)]
WGRAD_DIRECT_SHAPES = [(3, 2, 3), (2, 13, 17)]
WGRAD_SETTINGS = [(0.0, 1.0, None), (1.0, 1.0, None), (1.0, 2.0, 0.5), (1.0, 0.25, 0.5)]

# Mistakes a schedule can make (tests/test_ctx_reference_cpu.py proves that the stage check sees each of them) -> the
# gradients that own it, per form
WGRAD_MISTAKES = {
    "drop_dtu": dict(linear=("dW2",)),                     # the dt^T u term of dW2 left out
    "flip_dtu": dict(linear=("dW2",)),                     # ... or subtracted
    "scatter_rows": dict(linear=("dW2",)),                 # dW2cat's rows read as si * C + c instead of 4c + si
    "beta_twice": dict(linear=("dW2",)),                   # beta applied by the scatter AND the second term: 2 beta g0
    "scale_one_term": dict(linear=("dW2",)),               # scale * dscale on dG^T fv only
    "no_dscale": dict(linear=("dW1", "dW2"), direct=("dW1", "dW2")),
    "cells_swapped": dict(linear=("dW1", "dW2"), direct=("dW1",)),       # ave / u of scales 3 and 6 read transposed
    "cells_next_image": dict(linear=("dW1", "dW2"), direct=("dW1",)),    # ave / u taken from the next image
}


def wgrad_mistake_live(name, form, n, beta, scale, dscale):
    """Whether the mistake can be made at all in this case (and would change a gradient)."""
    if form not in WGRAD_MISTAKES[name]:
        return False
    if name == "beta_twice":
        return beta != 0.0
    if name == "scale_one_term":
        return scale * (1.0 if dscale is None else dscale) != 1.0
    if name == "no_dscale":
        return dscale is not None and dscale != 1.0
    if name == "cells_next_image":
        return n >= 2
    return True


def swap_cells(cells):
    """i and j swapped inside the cells of scales 3 and 6."""
    grids = cells_to_grids(cells)
    return grids_to_cells(grids[:2] + [g.transpose(2, 3) for g in grids[2:]])


def wgrad_stage(form, k, g0, beta, scale, dscale, mistake=None):
    """What the context backward leaves in the conv{S}_1 / conv{S}_2 gradient buffers, in fp64 -> (dW1, dW2), each
    [4, C, C]: beta g0 + scale dscale (fresh), from the kernels' own operands ``k``:
      linear form  dW1_S = du_all_S^T ave_S, dW2_S = dG_S^T fv + dt_S^T u_S   (dg [4, N, h, w, C] the stored 16-bit dG;
                   dt, u, du_all, ave the fp32 cell tables, du_all = du + W2^T dt)
      direct form  dW1_S = dA_S^T ave_S,     dW2_S = dz_S^T cs_S              (dz, cs [4, N, h, w, C]).
    g0 = (old dW1, old dW2), not read at beta = 0; dscale: a float or None.  mistake: a key of WGRAD_MISTAKES."""
    assert mistake is None or form in WGRAD_MISTAKES[mistake], (mistake, form)
    sd = scale * (1.0 if dscale is None or mistake == "no_dscale" else dscale)

    def cells(t):
        if mistake == "cells_swapped":
            return swap_cells(t)
        return t.roll(-1, 0) if mistake == "cells_next_image" else t
    ave = cells(k["ave"])
    if form == "linear":
        f1 = sd * wgrad_cells(k["du_all"], ave)
        a = wgrad_maps(k["dg"], k["fv"])
        if mistake == "scatter_rows":
            c = a.shape[1]
            a = a.permute(1, 0, 2).reshape(4 * c, c).reshape(4, c, c)     # dW2cat (rows 4c + si) read as [si][c]
        b = wgrad_cells(k["dt"], cells(k["u"]))
        b = {"drop_dtu": 0.0, "flip_dtu": -1.0}.get(mistake, 1.0) * b
        f2 = sd * a + (1.0 if mistake == "scale_one_term" else sd) * b
    else:
        f1 = sd * wgrad_cells(k["dA"], ave)
        f2 = sd * wgrad_maps(k["dz"], k["cs"])
    if beta == 0.0:
        return f1, f2
    return beta * g0[0].to(F64) + f1, (2.0 if mistake == "beta_twice" else 1.0) * beta * g0[1].to(F64) + f2


def wgrad_sum32_ratio(got, ref):
    """sum32_ratio of a stack of the four scales' weight gradients [4, C, C], scale by scale."""
    return max(sum32_ratio(got[si], ref[si]) for si in range(4))


# ------------------------------------------------------------------------------------------------------------- inputs
def structured_fv(n, h, w, c, dtype, seed, device="cpu"):
    """A post-ReLU feature map with spatial structure, [N, h, w, C] in the 16-bit ``dtype``: per image and channel a
    random affine ramp in y and x plus a y x term, a per-image offset (so the images of a batch differ in their pooled
    cells), noise of std 0.1, then ReLU (a non-trivial mask) and the rounding to ``dtype``.  Generated on the CPU
    from ``seed`` (the same values whatever the device)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, generator=g, dtype=F64)
    y = (torch.arange(h, dtype=F64) / max(h - 1, 1)).view(1, h, 1, 1)
    x = (torch.arange(w, dtype=F64) / max(w - 1, 1)).view(1, 1, w, 1)
    base = 0.3 + 0.5 * rnd(n, 1, 1, c)
    fv = base + rnd(n, 1, 1, c) * (y - 0.5) + rnd(n, 1, 1, c) * (x - 0.5) + rnd(n, 1, 1, c) * (y - 0.5) * (x - 0.5)
    fv = fv + 0.5 * rnd(n, 1, 1, 1) + 0.1 * rnd(n, h, w, c)
    return torch.relu(fv).to(dtype).to(device)


# ------------------------------------------------------------------------------------------------------------- checks
def out16_ratio(got, ref):
    """Worst err / bound of numerics.check_out16 at its default bound; <= 1 exactly when check_out16 passes."""
    g, r = got.to(F64), ref.to(F64)
    assert g.shape == r.shape, (g.shape, r.shape)
    rms = r.float().pow(2).mean().sqrt().item() + 1e-30
    return ((g - r).abs() / (RTOL16 * r.abs() + ATOL16_RMS * rms)).max().item()


def out16_outliers(got, ref):
    """How many elements numerics.check_out16 would report at its default bound."""
    g, r = got.to(F64), ref.to(F64)
    rms = r.float().pow(2).mean().sqrt().item() + 1e-30
    return int(((g - r).abs() > RTOL16 * r.abs() + ATOL16_RMS * rms).sum())


def sum32_ratio(got, ref, tol=1e-3):
    """Worst err / bound of numerics.check_sum32 at its default bound."""
    g, r = got.to(F64), ref.to(F64)
    assert g.shape == r.shape, (g.shape, r.shape)
    scale = r.abs().max().item() + 1e-30
    return ((g - r).abs() / (tol * (scale + r.abs()))).max().item()


def cells_sum32_ratio(got, ref):
    """sum32_ratio of a cell table [N, 50, C], scale by scale (each scale against its own max |ref|: the one cell of
    scale 1 sums the whole map and would otherwise set the bound of the 36 small cells of scale 6)."""
    return max(sum32_ratio(got[:, o:o + S * S], ref[:, o:o + S * S]) for S, o in zip(SCALES, CELL_OFF))


def pool_bound(fv, geo):
    """[N, 50, C]: the pooled cells' elementwise bound 4 K 2^-24 m, K the bin's pixel count and m the mean of |fv|
    over the bin (the kernel sums K fp32 products in two passes; leaving one pixel out moves a cell by |x| / K)."""
    g = Geometry(geo.h, geo.w, fv.device)             # always the true bins, whatever geometry is under test
    m = pool_cells(fv.to(F64).abs(), g)
    return 4.0 * cell_pixels(g, fv.device)[None, :, None] * 2.0 ** -24 * m


def pool_ratio(got, fv, geo, ref=None):
    """Worst err / pool_bound of pooled cells ``got`` (0 / 0 counts as 0: an all-zero bin must pool to exactly 0)."""
    ref = pool_cells(fv, Geometry(geo.h, geo.w, fv.device)) if ref is None else ref
    err = (got.to(F64) - ref).abs()
    bound = pool_bound(fv, geo)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return ratio.max().item()
