"""The multi-scale context module's schedule inside the native executor (reference: model/CANNet.py:39-87, the four
scales S in {1, 2, 3, 6} of adaptive avg-pool -> conv{S}_1 -> bilinear upsample -> (s - fv) -> conv{S}_2 -> sigmoid,
fused as fi = sum w s / (sum w + 1e-12) and concatenated with fv).

Two forms, picked per map by ``_ctx_linear``:
  * linearised (default): conv{S}_2 and the bilinear upsample are both linear per channel, so
    z_S = conv{S}_2(up(u_S) - fv) = up(W2_S u_S) - W2_S fv: one GEMM over fv with the four W2_S interleaved into 2048
    output columns (conv_igemm.hip EPI_CTXF: the epilogue upsamples the S x S cell tables, applies the sigmoid, forms
    fi and writes fv | fi into the concat buffer), one GEMM back (EPI_CTXB), fp32 cell GEMMs (ctx_gemm) for the
    50 pooled cells; the expanded maps c_S and their sigmoid maps never exist;
  * direct (maps narrower than 64 columns or of fewer than 3 rows at 1/8 resolution, or dispatch ctx_linear = 0):
    expand the four c_S maps, four sigmoid GEMMs in one batched launch, fuse.

``ContextSchedule`` is a mixin of ops.executor.CANNetExecutor (it uses the executor's packs, streams and side-stream
fork helpers).
"""
from __future__ import annotations

import torch

from . import conv as C
from . import dispatch
from ..models.cannet import CONTEXT_SCALES


class ContextSchedule:
    # ----------------------------------------------------------- forward
    @staticmethod
    def _ctx_linear(fv) -> bool:
        """The context module as one GEMM each way (conv_igemm.hip "Linearised context module"); dispatch ctx_linear =
        0, a map narrower than 64 columns or one of fewer than 3 rows: the direct per-scale form (expand -> 4 sigmoid
        GEMMs -> fuse)."""
        return bool(dispatch.current().ctx_linear) and C.ctx_linear_ok(fv)

    def _context_fwd(self, fv, save, wv=None):
        if self._ctx_linear(fv):
            return self._context_fwd_linear(fv, save, wv)
        if wv is not None:
            raise ValueError("a width-padded map needs the linearised context module")
        n, h, w, c = fv.shape
        st = self._stream()
        rowacc = torch.empty(n, h, 12, c, dtype=torch.float32, device=fv.device)
        ave = torch.empty(n, 50, c, dtype=torch.float32, device=fv.device)
        self.C.ctx_reduce(0, fv.data_ptr(), 0, 0, rowacc.data_ptr(), ave.data_ptr(), n, h, w, c, self.dt, st)
        # conv{S}_1 on the pooled grids: the four scales' fp32 GEMMs in one launch
        table = torch.empty_like(ave)
        self.C.ctx_gemm(0, ave.data_ptr(), 0, self._ctx1_ptrs(), table.data_ptr(), [], n, c, 0.0, 1.0, 0, st)
        cs = torch.empty(4, n, h, w, c, dtype=self.act, device=fv.device)
        self.C.ctx_expand(fv.data_ptr(), table.data_ptr(), cs.data_ptr(), n, h, w, c, self.dt, st)
        wts = torch.empty(4, n, h, w, c, dtype=self.act, device=fv.device)
        if self._ctx_batched(h, w):
            C.conv_igemm_batched(cs, self.ctx2_fwd, ksize=1, epi=C.EPI_SIGMOID, out=wts)   # one launch
        else:
            for i, sc in enumerate(CONTEXT_SCALES):
                fwd, _ = self.packs[id(self.ctx2[sc].weight)]
                C.conv_igemm(cs[i], fwd, None, ksize=1, epi=C.EPI_SIGMOID, out=wts[i])
        cat = torch.empty(n, h, w, 2 * c, dtype=self.act, device=fv.device)
        self.C.ctx_fuse(fv.data_ptr(), wts.data_ptr(), table.data_ptr(), cat.data_ptr(), n, h, w, c, self.dt, st)
        saved = dict(ave=ave, table=table, cs=cs, wts=wts, rowacc=rowacc) if save else None
        return cat, saved

    def _context_fwd_linear(self, fv, save, wv=None):
        n, h, w, c = fv.shape
        st = self._stream()
        rowacc = torch.empty(n, h, 12, c, dtype=torch.float32, device=fv.device)
        ave = torch.empty(n, 50, c, dtype=torch.float32, device=fv.device)
        self.C.ctx_reduce(0, fv.data_ptr(), 0, 0, rowacc.data_ptr(), ave.data_ptr(), n, h, w, c, self.dt, st,
                          wv or 0)
        u = torch.empty_like(ave)            # conv{S}_1 on the pooled cells
        self.C.ctx_gemm(0, ave.data_ptr(), 0, self._ctx1_ptrs(), u.data_ptr(), [], n, c, 0.0, 1.0, 0, st)
        t = torch.empty_like(ave)            # conv{S}_2 on the same cells (its upsample is z's first term)
        self.C.ctx_gemm(0, u.data_ptr(), 0, self._ctx2_ptrs(), t.data_ptr(), [], n, c, 0.0, 1.0, 0, st)
        wts, cat = C.conv_ctx_fwd(fv, self.ctx2cat_fwd, t, u, wvalid=wv)
        saved = dict(linear=True, ave=ave, u=u, wts=wts, wv=wv) if save else None
        return cat, saved

    def _ctx2_ptrs(self):
        ws = [self.ctx2[sc].weight for sc in CONTEXT_SCALES]
        for w_ in ws:
            if not (w_.is_contiguous() and w_.dtype == torch.float32):
                raise ValueError("conv{S}_2 weights must be contiguous fp32")
        return [w_.data_ptr() for w_ in ws]

    @staticmethod
    def _ctx_batched(h, w):
        """The four conv{S}_2 1x1 convs as one batched launch (maps of at least 2 x 2)."""
        return h >= 2 and w >= 2

    def _ctx1_ptrs(self):
        ws = [self.ctx1[sc].weight for sc in CONTEXT_SCALES]
        for w_ in ws:
            if not (w_.is_contiguous() and w_.dtype == torch.float32):
                raise ValueError("conv{S}_1 weights must be contiguous fp32")
        return [w_.data_ptr() for w_ in ws]

    # ----------------------------------------------------------- backward
    def _context_bwd_linear(self, ctx, fv, dcat, grads, ws, beta, scale, ready, dscale=None, side=None, hold=None):
        """Backward of the linearised context module (see _context_fwd_linear); returns d(F10 pre-activation)."""
        st = self._stream()
        n, h, w, c = fv.shape
        hold = [] if hold is None else hold
        wv = ctx.get("wv")
        dg, rowacc = C.ctx_bwd_lin(dcat, ctx["wts"], ctx["u"], wvalid=wv)   # dG = -dz, x-pass partials of up^T
        dt = torch.empty(n, 50, c, dtype=torch.float32, device=fv.device)
        du = torch.empty_like(dt)
        # dt_S = up^T(dz_S) and du_S = up^T(ds_S) (direct part), one launch
        self.C.ctx_cells(rowacc[0].data_ptr(), dt.data_ptr(), n, h, c, st, rowacc[1].data_ptr(), du.data_ptr())
        u, ave = ctx["u"], ctx["ave"]
        dw2 = [grads[self.ctx2_index[sc]] for sc in CONTEXT_SCALES]
        for g in dw2:
            if not (g.is_contiguous() and g.dtype == torch.float32):
                raise ValueError("conv{S}_2 gradient buffers must be contiguous fp32")
        if getattr(self, "_dw2cat", None) is None or self._dw2cat.device != fv.device:
            self._dw2cat = torch.empty(4 * c, c, 1, 1, dtype=torch.float32, device=fv.device)
        dw2cat = self._dw2cat
        dsp = dscale.data_ptr() if dscale is not None else 0

        # du_S += W2_S^T dt_S, then dave_S = W1_S^T du_S (fp32 cell GEMMs).  Both before the side-stream fork:
        # forked first, the dW2cat weight gradient takes every CU (one 128-KB-LDS block each) and these two short
        # launches wait ~190 us behind it on the critical path
        self.C.ctx_gemm(1, dt.data_ptr(), 0, self._ctx2_ptrs(), du.data_ptr(), [], n, c, 1.0, 1.0, 0, st)
        dave = torch.empty_like(du)
        self.C.ctx_gemm(1, du.data_ptr(), 0, self._ctx1_ptrs(), dave.data_ptr(), [], n, c, 0.0, 1.0, 0, st)

        def ctx2_wgrad():
            # dW2_S = dG_S^T fv (one GEMM over the interleaved columns) + dt_S^T u_S (the t = W2 u term)
            C.conv_wgrad(dg, fv, dw2cat, None, ksize=1, ws=ws, beta=0.0, scale=scale, dscale=dscale)
            self.C.ctx_w2_scatter(dw2cat.data_ptr(), [g.data_ptr() for g in dw2], c, float(beta), self._stream())
            self.C.ctx_gemm(2, dt.data_ptr(), u.data_ptr(), [], 0, [g.data_ptr() for g in dw2], n, c, 1.0,
                            float(scale), dsp, self._stream())
            ready([self.ctx2_index[sc] for sc in CONTEXT_SCALES])
        self._on_side(side, ctx2_wgrad, hold, dg, fv, dt, u)

        def ctx1_wgrad():
            gws = [grads[self.ctx1_index[sc]] for sc in CONTEXT_SCALES]
            for g in gws:
                if not (g.is_contiguous() and g.dtype == torch.float32):
                    raise ValueError("conv{S}_1 gradient buffers must be contiguous fp32")
            self.C.ctx_gemm(2, du.data_ptr(), ave.data_ptr(), [], 0, [g.data_ptr() for g in gws], n, c, float(beta),
                            float(scale), dsp, self._stream())
            ready([self.ctx1_index[sc] for sc in CONTEXT_SCALES])
        self._on_side(side, ctx1_wgrad, hold, du, ave)
        hold.append(rowacc)
        return C.conv_ctx_bwd(dg, self.ctx2cat_dgr, dave, dcat, fv, wvalid=wv)

    def _context_bwd(self, ctx, fv, dcat, grads, ws, beta, scale, ready, dscale=None, side=None, hold=None):
        """Backward of the context module; returns d(F10 pre-activation) (ReLU mask of fv applied)."""
        if ctx.get("linear"):
            return self._context_bwd_linear(ctx, fv, dcat, grads, ws, beta, scale, ready, dscale, side, hold)
        st = self._stream()
        n, h, w, c = fv.shape
        dz = torch.empty(4, n, h, w, c, dtype=self.act, device=fv.device)
        sdir = torch.empty_like(dz)
        self.C.ctx_bwd_e1(dcat.data_ptr(), ctx["wts"].data_ptr(), ctx["table"].data_ptr(), dz.data_ptr(),
                          sdir.data_ptr(), n, h, w, c, self.dt, st)
        dc = torch.empty_like(dz)
        if self._ctx_batched(h, w):
            C.conv_igemm_batched(dz, self.ctx2_dgr, ksize=1, epi=C.EPI_NONE, out=dc)
        else:
            for i, sc in enumerate(CONTEXT_SCALES):
                _, dgr = self.packs[id(self.ctx2[sc].weight)]
                C.conv_igemm(dz[i], dgr, None, ksize=1, epi=C.EPI_NONE, out=dc[i])
        # the four conv{S}_2 weight gradients: one batched GEMM when their arena slots are adjacent
        dws = [grads[self.ctx2_index[sc]] for sc in CONTEXT_SCALES]

        def ctx2_wgrad():
            if C.wgrad_1x1_batched_ok(dz, ctx["cs"], dws):
                C.conv_wgrad_1x1_batched(dz, ctx["cs"], dws, ws=ws, beta=beta, scale=scale, dscale=dscale)
            else:
                for i, sc in enumerate(CONTEXT_SCALES):
                    C.conv_wgrad(dz[i], ctx["cs"][i], dws[i], None, ksize=1, ws=ws, beta=beta, scale=scale,
                                 dscale=dscale)
            ready([self.ctx2_index[sc] for sc in CONTEXT_SCALES])
        hold = [] if hold is None else hold
        self._on_side(side, ctx2_wgrad, hold, dz)
        rowacc = ctx["rowacc"]
        dA = torch.empty(n, 50, c, dtype=torch.float32, device=fv.device)
        self.C.ctx_reduce(1, 0, sdir.data_ptr(), dc.data_ptr(), rowacc.data_ptr(), dA.data_ptr(), n, h, w, c, self.dt,
                          st)
        dave = torch.empty_like(dA)
        ave = ctx["ave"]

        def ctx1_wgrad():
            # dW1_S = dA_S^T @ ave_S for the four scales, one launch (on the weight-gradient stream)
            gws = [grads[self.ctx1_index[sc]] for sc in CONTEXT_SCALES]
            for g in gws:
                if not (g.is_contiguous() and g.dtype == torch.float32):
                    raise ValueError("conv{S}_1 gradient buffers must be contiguous fp32")
            self.C.ctx_gemm(2, dA.data_ptr(), ave.data_ptr(), [], 0, [g.data_ptr() for g in gws], n, c, float(beta),
                            float(scale), dscale.data_ptr() if dscale is not None else 0, self._stream())
            ready([self.ctx1_index[sc] for sc in CONTEXT_SCALES])
        self._on_side(side, ctx1_wgrad, hold, dA, ave)
        self.C.ctx_gemm(1, dA.data_ptr(), 0, self._ctx1_ptrs(), dave.data_ptr(), [], n, c, 0.0, 1.0, 0, st)
        dfv = torch.empty(n, h, w, c, dtype=self.act, device=fv.device)
        self.C.ctx_bwd_final(dcat.data_ptr(), dc.data_ptr(), dave.data_ptr(), fv.data_ptr(), dfv.data_ptr(), n, h, w,
                             c, self.dt, st)
        return dfv
