"""Numerics of the MFMA implicit-GEMM conv kernels vs a plain fp32 PyTorch reference."""
import pytest
import torch
import torch.nn.functional as F
from numerics import check, check_out16

pytestmark = pytest.mark.gpu


def _ref(x_nhwc, w, b, dil, relu=True):
    x = x_nhwc.float().permute(0, 3, 1, 2)
    pad = dil * (w.shape[-1] // 2)
    y = F.conv2d(x, w.float(), b, padding=pad, dilation=dil)
    if relu:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1)


def _close(a, b):
    """Tight elementwise check (tests/numerics.py): 16-bit outputs to 8e-3 relative + 2e-3 rms, fp32 weight
    gradients to 1e-3 of (max + |value|)."""
    check(a, b)


@pytest.mark.parametrize("n,h,w,ci,co,k,dil,tile", [
    (2, 24, 40, 64, 64, 3, 1, 0), (1, 17, 33, 128, 128, 3, 1, 0), (2, 32, 32, 256, 512, 3, 2, 0),
    (1, 12, 16, 1024, 512, 3, 2, 0), (2, 16, 24, 512, 512, 1, 1, 0),
    (1, 20, 20, 128, 256, 3, 1, 1), (1, 20, 20, 128, 256, 3, 1, 2), (1, 20, 20, 128, 256, 3, 1, 3),
    (1, 20, 20, 128, 256, 3, 1, 4),
    (1, 20, 20, 128, 256, 3, 1, 11), (1, 20, 20, 128, 256, 3, 1, 12), (1, 20, 20, 128, 256, 3, 1, 13),
    (2, 9, 13, 64, 128, 3, 2, 0), (1, 7, 5, 512, 1024, 3, 2, 0), (3, 11, 17, 64, 64, 3, 1, 0),
    # v2 pipelined LDS-DMA kernel: every tile, 1x1 (nk = Cin/64), nk = 1, nk = 2, dilation 2, ragged M
    (1, 20, 20, 128, 256, 3, 1, 21), (1, 20, 20, 128, 256, 3, 1, 22), (1, 20, 20, 128, 256, 3, 1, 23),
    (2, 16, 24, 512, 512, 1, 1, 21), (1, 9, 13, 64, 256, 1, 1, 21), (1, 9, 13, 128, 128, 1, 1, 22),
    (2, 32, 32, 256, 512, 3, 2, 21), (3, 11, 17, 64, 64, 3, 1, 23), (2, 9, 13, 64, 128, 3, 2, 22),
    # halo-tiled Cin = 64 kernel: full tiles, ragged rows / columns, Cout 64 and 128
    (1, 4, 128, 64, 64, 3, 1, 31), (2, 10, 200, 64, 64, 3, 1, 31), (1, 9, 130, 64, 128, 3, 1, 31),
    (2, 3, 7, 64, 128, 3, 1, 31),
    # 128 x 512 tile (160 KB LDS)
    (1, 20, 40, 128, 128, 3, 1, 25), (2, 9, 13, 256, 128, 3, 2, 25), (1, 5, 7, 128, 384, 1, 1, 25),
])
def test_conv_fwd(n, h, w, ci, co, k, dil, tile):
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(0)
    dev = "cuda"
    x = torch.randn(n, h, w, ci, device=dev).to(torch.bfloat16)
    wt = (torch.randn(co, ci, k, k, device=dev) * 0.05).to(torch.bfloat16).float()
    b = torch.randn(co, device=dev)
    y = C.conv_igemm(x, C.pack_weight_fwd(wt), b, ksize=k, dil=dil, tile=tile)
    torch.cuda.synchronize()
    _close(y, _ref(x, wt, b, dil))


@pytest.mark.parametrize("n,h,w,tile", [(2, 40, 56, 0), (1, 37, 150, 0), (2, 8, 256, 0), (2, 40, 56, 32),
                                        (3, 200, 640, 0)])
def test_conv_first_layer(n, h, w, tile):
    """tile 0 (auto) / 32: halo-tiled first-layer kernel (persistent, prefetching the next tile's halo; the last
    shape has more tiles than two per CU, so blocks walk several)."""
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(1)
    img = torch.randn(n, 3, h, w, device="cuda")
    wt = (torch.randn(64, 3, 3, 3, device="cuda") * 0.2).to(torch.bfloat16).float()
    b = torch.randn(64, device="cuda")
    x4 = C.to_nhwc4(img)
    y = C.conv_igemm(x4, C.pack_weight_first(wt), b, ksize=3, first=True, tile=tile)
    ref = _ref(x4[..., :3].contiguous(), wt, b, 1)
    _close(y, ref)


@pytest.mark.parametrize("n,h,w,ci,co,dil,tile", [
    (2, 24, 40, 64, 128, 1, 0), (1, 16, 16, 512, 1024, 2, 0), (1, 9, 13, 64, 64, 1, 0),
    (1, 16, 16, 512, 1024, 2, 21), (2, 24, 40, 128, 64, 1, 22), (1, 9, 13, 64, 64, 1, 23),
    (2, 9, 140, 64, 64, 1, 31), (1, 12, 256, 128, 64, 1, 31)])
def test_conv_dgrad_mask(n, h, w, ci, co, dil, tile):
    """dX = conv_transpose(dY, W) * (mask > 0) via the same kernel with the flipped pack."""
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(2)
    dev = "cuda"
    wt = (torch.randn(co, ci, 3, 3, device=dev) * 0.05).to(torch.bfloat16).float()
    dy = torch.randn(n, h, w, co, device=dev).to(torch.bfloat16)
    mask = torch.randn(n, h, w, ci, device=dev).to(torch.bfloat16)
    dx = C.conv_igemm(dy, C.pack_weight_dgrad(wt), None, ksize=3, dil=dil, epi=C.EPI_MASK, mask=mask, tile=tile)
    xr = torch.zeros(n, ci, h, w, device=dev, requires_grad=True)
    y = F.conv2d(xr, wt, None, padding=dil, dilation=dil)
    (gx,) = torch.autograd.grad(y, xr, dy.float().permute(0, 3, 1, 2))
    ref = gx.permute(0, 2, 3, 1) * (mask.float() > 0)
    _close(dx, ref)


@pytest.mark.parametrize("n,h,w,ci,co,k,dil", [
    (2, 24, 40, 64, 64, 3, 1), (1, 17, 33, 128, 128, 3, 1), (2, 16, 16, 256, 512, 3, 2),
    (1, 12, 16, 128, 64, 3, 2), (2, 16, 24, 512, 512, 1, 1), (1, 40, 40, 64, 128, 3, 1),
    (1, 7, 9, 256, 256, 3, 2), (2, 13, 11, 64, 64, 3, 1), (1, 9, 10, 1024, 512, 3, 2), (1, 6, 8, 128, 256, 3, 1),
])
def test_conv_wgrad(n, h, w, ci, co, k, dil):
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(3)
    dev = "cuda"
    x = torch.randn(n, h, w, ci, device=dev).to(torch.bfloat16)
    dy = torch.randn(n, h, w, co, device=dev).to(torch.bfloat16)
    dw = torch.empty(co, ci, k, k, device=dev)
    db = torch.empty(co, device=dev)
    C.conv_wgrad(dy, x, dw, db, ksize=k, dil=dil)
    wr = torch.zeros(co, ci, k, k, device=dev, requires_grad=True)
    br = torch.zeros(co, device=dev, requires_grad=True)
    y = F.conv2d(x.float().permute(0, 3, 1, 2), wr, br, padding=dil * (k // 2), dilation=dil)
    gw, gb = torch.autograd.grad(y, (wr, br), dy.float().permute(0, 3, 1, 2))
    _close(dw, gw)
    _close(db, gb)


@pytest.mark.parametrize("n,h,w,ci,co,dil,bias", [
    (1, 6, 64, 256, 256, 1, True), (2, 5, 128, 512, 256, 2, True), (1, 3, 64, 1024, 512, 2, True),
    (3, 4, 64, 256, 512, 1, False), (1, 2, 64, 512, 512, 2, True),
    # ragged widths (W % 64 != 0, odd H): virtual 64-pixel stages per row, the padding pixels read zeros
    (2, 7, 100, 256, 256, 1, True), (1, 9, 120, 512, 256, 2, True), (3, 5, 30, 256, 512, 1, False),
    (1, 4, 135, 1024, 512, 2, True)])
def test_conv_wgrad_v2_row_aligned(n, h, w, ci, co, dil, bias, dispatch_cfg):
    """W % 64 == 0, Cin % 256 == 0 layers take the v2 pipelined wgrad (cfg 9) with bias column-sum blocks (with the
    tap-ring kernel off: it takes these layers by default)."""
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops import conv as C
    dispatch_cfg(wgrad_tap=0)
    assert _ext.require().wgrad_plan(n * h * w, ci, co, 3, 0, 1024, dil, w)[2] == 9
    plan = _ext.require().wgrad_launch_plan(n, h, w, n * h * w, ci, co, 3, dil, want_db=bias)
    assert (plan["cfg"], plan["family"], plan["ragged"]) == (9, 2, w % 64 != 0), plan     # family 2: the v2 kernel
    torch.manual_seed(6)
    x = torch.randn(n, h, w, ci, device="cuda").to(torch.bfloat16)
    dy = torch.randn(n, h, w, co, device="cuda").to(torch.bfloat16)
    dw = torch.empty(co, ci, 3, 3, device="cuda")
    db = torch.empty(co, device="cuda") if bias else None
    C.conv_wgrad(dy, x, dw, db, ksize=3, dil=dil)
    wr = torch.zeros(co, ci, 3, 3, device="cuda", requires_grad=True)
    br = torch.zeros(co, device="cuda", requires_grad=True)
    y = F.conv2d(x.float().permute(0, 3, 1, 2), wr, br, padding=dil, dilation=dil)
    gw, gb = torch.autograd.grad(y, (wr, br), dy.float().permute(0, 3, 1, 2))
    _close(dw, gw)
    if bias:
        _close(db, gb)


@pytest.mark.parametrize("n,h,w,ci,co,dil,dtype", [
    (1, 6, 64, 64, 128, 1, torch.bfloat16), (2, 7, 128, 128, 256, 1, torch.bfloat16),
    (1, 9, 120, 256, 128, 2, torch.bfloat16), (2, 5, 200, 64, 256, 2, torch.float16),
    (1, 12, 96, 512, 512, 2, torch.bfloat16), (3, 4, 64, 128, 128, 1, torch.float16),
    (1, 1, 64, 64, 128, 1, torch.bfloat16), (1, 3, 40, 64, 128, 2, torch.bfloat16),
    # 1024 -> 512: 64 tiles, 4 slices over 36 stages -> slices that span chains (several segments each)
    (2, 9, 128, 1024, 512, 2, torch.bfloat16),
    # Cout = 64: the 64-channel tile (4 waves, two blocks per CU, 2-stage DMA lead)
    (1, 6, 64, 64, 64, 1, torch.bfloat16), (2, 9, 120, 128, 64, 2, torch.bfloat16),
    (1, 5, 200, 64, 64, 1, torch.float16), (3, 16, 256, 64, 64, 1, torch.bfloat16)])
def test_wgrad_tap_ring(n, h, w, ci, co, dil, dtype, dispatch_cfg):
    """Tap-ring weight gradient (cfg 12: 128 output channels x 9 taps of a 64-channel input slice, input rows in an
    LDS ring walked down 64-column chains, one chain per row phase for dilation 2) == the fp32 reference: ragged
    widths (W % 64 != 0) and heights, single-row maps, slices spanning several chains, bias through the column-sum
    path."""
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops import conv as C
    dispatch_cfg(wgrad_tap=3)
    assert _ext.require().wgrad_plan(n * h * w, ci, co, 3, 0, 1024, dil, w)[2] == 12
    torch.manual_seed(16)
    x = torch.randn(n, h, w, ci, device="cuda").to(dtype)
    dy = torch.randn(n, h, w, co, device="cuda").to(dtype)
    dw = torch.empty(co, ci, 3, 3, device="cuda")
    db = torch.empty(co, device="cuda")
    C.conv_wgrad(dy, x, dw, db, ksize=3, dil=dil)
    torch.cuda.synchronize()
    wr = torch.zeros(co, ci, 3, 3, device="cuda", requires_grad=True)
    br = torch.zeros(co, device="cuda", requires_grad=True)
    y = F.conv2d(x.float().permute(0, 3, 1, 2), wr, br, padding=dil, dilation=dil)
    gw, gb = torch.autograd.grad(y, (wr, br), dy.float().permute(0, 3, 1, 2))
    _close(dw, gw)
    _close(db, gb)


def test_conv_wgrad_first_layer():
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(4)
    img = torch.randn(2, 3, 40, 56, device="cuda")
    x4 = C.to_nhwc4(img)
    dy = torch.randn(2, 40, 56, 64, device="cuda").to(torch.bfloat16)
    dw = torch.empty(64, 3, 3, 3, device="cuda")
    db = torch.empty(64, device="cuda")
    C.conv_wgrad(dy, x4, dw, db, ksize=3, first=True)
    wr = torch.zeros(64, 3, 3, 3, device="cuda", requires_grad=True)
    br = torch.zeros(64, device="cuda", requires_grad=True)
    y = F.conv2d(x4[..., :3].float().permute(0, 3, 1, 2), wr, br, padding=1)
    gw, gb = torch.autograd.grad(y, (wr, br), dy.float().permute(0, 3, 1, 2))
    _close(dw, gw)
    _close(db, gb)


@pytest.mark.parametrize("n,h,w,ci,co", [(1, 256, 1024, 64, 64), (2, 181, 733, 128, 128), (1, 301, 900, 64, 128)])
def test_conv_wgrad_halo_path(n, h, w, ci, co, dispatch_cfg):
    """Large-M, small-channel layers off the tap ring take the row-ring halo wgrad kernel, 4-row tiles down
    64-column strips (odd H, W not a multiple of 64 included: the general-addressing kernel); the last two shapes
    have slices that cross strip boundaries (full-halo reload mid-slice) and a ragged last tile row."""
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops import conv as C
    dispatch_cfg(wgrad_tap=0)
    assert _ext.require().wgrad_plan(n * h * w, ci, co, 3, 0, 1024, 1, w)[2] == 8
    torch.manual_seed(5)
    x = torch.randn(n, h, w, ci, device="cuda").to(torch.bfloat16)
    dy = torch.randn(n, h, w, co, device="cuda").to(torch.bfloat16)
    dw = torch.empty(co, ci, 3, 3, device="cuda")
    db = torch.empty(co, device="cuda")
    C.conv_wgrad(dy, x, dw, db, ksize=3, dil=1)
    wr = torch.zeros(co, ci, 3, 3, device="cuda", requires_grad=True)
    br = torch.zeros(co, device="cuda", requires_grad=True)
    y = F.conv2d(x.float().permute(0, 3, 1, 2), wr, br, padding=1)
    gw, gb = torch.autograd.grad(y, (wr, br), dy.float().permute(0, 3, 1, 2))
    _close(dw, gw)
    _close(db, gb)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w,ci,co", [(2, 128, 1024, 64, 64), (1, 512, 576, 128, 128), (4, 96, 704, 64, 128)])
def test_ring_wgrad_fast_addressing(n, h, w, ci, co, dtype, dispatch_cfg):
    """Row-ring weight gradient with the hoisted, skewed DMA addressing (H % 4 == 0, W % 64 == 0: per-lane offsets
    from the tile / row origins, edge slots zeroed per lane): several strips per image, several images, 2 ci / co
    tiles, slices crossing strips; repeatable bit for bit, and == the fp32 reference where it fits."""
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops import conv as C
    dispatch_cfg(wgrad_tap=0)
    assert _ext.require().wgrad_plan(n * h * w, ci, co, 3, 0, 1024, 1, w)[2] == 8
    torch.manual_seed(21)
    x = torch.randn(n, h, w, ci, device="cuda").to(dtype)
    dy = torch.randn(n, h, w, co, device="cuda").to(dtype)
    dw0, db0 = torch.empty(co, ci, 3, 3, device="cuda"), torch.empty(co, device="cuda")
    dw1, db1 = torch.empty_like(dw0), torch.empty_like(db0)
    ws = C.WgradWorkspace("cuda")
    C.conv_wgrad(dy, x, dw0, db0, ksize=3, dil=1, ws=ws)
    C.conv_wgrad(dy, x, dw1, db1, ksize=3, dil=1, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
    if n * h * w <= 300000:
        wr = torch.zeros(co, ci, 3, 3, device="cuda", requires_grad=True)
        br = torch.zeros(co, device="cuda", requires_grad=True)
        y = F.conv2d(x.float().permute(0, 3, 1, 2), wr, br, padding=1)
        gw, gb = torch.autograd.grad(y, (wr, br), dy.float().permute(0, 3, 1, 2))
        _close(dw0, gw)
        _close(db0, gb)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_conv_wgrad_1x1_batched(dtype):
    """The four context-module 1x1 weight gradients in one batched launch == fp32 reference, per item."""
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(7)
    nb, n, h, w, c = 4, 2, 12, 128, 512
    dy = torch.randn(nb, n, h, w, c, device="cuda").to(dtype)
    x = torch.randn(nb, n, h, w, c, device="cuda").to(dtype)
    arena = torch.full((nb * c * c,), float("nan"), device="cuda")
    dws = [arena[i * c * c:(i + 1) * c * c].view(c, c, 1, 1) for i in range(nb)]
    assert C.wgrad_1x1_batched_ok(dy, x, dws)
    ws = C.WgradWorkspace("cuda")
    C.conv_wgrad_1x1_batched(dy, x, dws, ws=ws, scale=0.5)
    for b in range(nb):
        ref = 0.5 * dy[b].float().reshape(-1, c).t() @ x[b].float().reshape(-1, c)
        _close(dws[b].view(c, c), ref)


_SENTINEL = 7.0


@pytest.mark.parametrize("rows,cols,cfg", [(6, 8, 1), (6, 64, 12)])
def test_conv_wgrad_refuses_a_short_workspace(rows, cols, cfg, dispatch_cfg):
    """The launcher plans its own launch and is told the workspace's size: one float short of the plan's need it
    returns -21 before anything is launched (dw, db and the workspace keep their sentinel); with the whole need it
    runs, and gives the front end's result bit for bit.  cfg 1: LDS-DMA GEMM; cfg 12: tap ring."""
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops import conv as C
    ext = _ext.require()
    dispatch_cfg(wgrad_tap=3 if cfg == 12 else 0)
    ci, co = 64, 128
    _, _, got, need = C.WgradWorkspace("cuda").plan(rows * cols, ci, co, 3, False, 1, cols)
    assert got == cfg
    torch.manual_seed(9)
    x = torch.randn(1, rows, cols, ci, device="cuda").to(torch.bfloat16)
    dy = torch.randn(1, rows, cols, co, device="cuda").to(torch.bfloat16)
    buf = torch.full((need,), _SENTINEL, device="cuda")
    dw, db = torch.full((co, ci, 3, 3), _SENTINEL, device="cuda"), torch.full((co,), _SENTINEL, device="cuda")

    def launch(ws_floats):
        ext.conv_wgrad(dy.data_ptr(), x.data_ptr(), buf.data_ptr(), ws_floats, dw.data_ptr(), db.data_ptr(), 1, rows,
                       cols, ci, co, 3, 1, 0, 0.0, 1.0, 0, C.dt_code(dy.dtype), _ext.stream_ptr(x.device))

    with pytest.raises(RuntimeError, match="rc=-21"):
        launch(need - 1)
    torch.cuda.synchronize()
    assert bool((dw == _SENTINEL).all()) and bool((db == _SENTINEL).all()) and bool((buf == _SENTINEL).all())
    launch(need)
    dw2, db2 = torch.empty_like(dw), torch.empty_like(db)
    C.conv_wgrad(dy, x, dw2, db2, ksize=3)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def test_conv_wgrad_1x1_batched_refuses_a_short_workspace():
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops import conv as C
    ext = _ext.require()
    nb, h, w, c = 4, 2, 64, 256
    m = h * w
    ncu = C._ctx_wgrad_cus()
    need = C.wgrad_1x1_batched_plan(m, nb, c, c)[2]
    torch.manual_seed(10)
    x = torch.randn(nb, 1, h, w, c, device="cuda").to(torch.bfloat16)
    dy = torch.randn(nb, 1, h, w, c, device="cuda").to(torch.bfloat16)
    buf = torch.full((need,), _SENTINEL, device="cuda")
    arena = torch.full((nb * c * c,), _SENTINEL, device="cuda")
    with pytest.raises(RuntimeError, match="rc=-21"):
        ext.conv_wgrad_1x1_batched(dy.data_ptr(), x.data_ptr(), buf.data_ptr(), need - 1, arena.data_ptr(), m, w, c, c,
                                   nb, m * c, m * c, c * c, ncu, 0.0, 1.0, 0, C.dt_code(dy.dtype),
                                   _ext.stream_ptr(x.device))
    torch.cuda.synchronize()
    assert bool((arena == _SENTINEL).all()) and bool((buf == _SENTINEL).all())


@pytest.mark.parametrize("n,h,w,ci,co,dil,cfg,bias", [
    (1, 6, 64, 128, 256, 1, 10, True), (2, 5, 128, 128, 512, 2, 10, False), (1, 9, 64, 256, 128, 2, 11, True),
    (2, 4, 64, 512, 128, 1, 11, True),
    # ragged widths (W % 64 != 0): virtual 64-pixel stages per row, padding pixels zero
    (1, 6, 90, 128, 256, 1, 10, True), (2, 5, 100, 512, 128, 2, 11, True)])
def test_conv_wgrad_v2_half_tiles(n, h, w, ci, co, dil, cfg, bias, dispatch_cfg):
    """v2 pipelined wgrad with 256co x 128k (Cin = 128, cfg 10) and 128co x 256k (Cout = 128, cfg 11) tiles (tap-ring
    kernel off)."""
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops import conv as C
    dispatch_cfg(wgrad_tap=0)
    assert _ext.require().wgrad_plan(n * h * w, ci, co, 3, 0, 1024, dil, w)[2] == cfg
    plan = _ext.require().wgrad_launch_plan(n, h, w, n * h * w, ci, co, 3, dil, want_db=bias)
    assert (plan["cfg"], plan["family"], plan["ragged"]) == (cfg, 2, w % 64 != 0), plan   # family 2: the v2 kernel
    torch.manual_seed(8)
    x = torch.randn(n, h, w, ci, device="cuda").to(torch.bfloat16)
    dy = torch.randn(n, h, w, co, device="cuda").to(torch.bfloat16)
    dw = torch.empty(co, ci, 3, 3, device="cuda")
    db = torch.empty(co, device="cuda") if bias else None
    C.conv_wgrad(dy, x, dw, db, ksize=3, dil=dil)
    wr = torch.zeros(co, ci, 3, 3, device="cuda", requires_grad=True)
    br = torch.zeros(co, device="cuda", requires_grad=True)
    y = F.conv2d(x.float().permute(0, 3, 1, 2), wr, br, padding=dil, dilation=dil)
    gw, gb = torch.autograd.grad(y, (wr, br), dy.float().permute(0, 3, 1, 2))
    _close(dw, gw)
    if bias:
        _close(db, gb)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w,ci,co,dil", [(2, 8, 512, 128, 128, 1), (1, 6, 256, 256, 256, 1),
                                             (2, 4, 256, 256, 128, 2), (1, 4, 512, 128, 64, 1),
                                             (2, 8, 128, 64, 64, 1), (1, 12, 320, 64, 64, 1)])
def test_conv_pool_fwd_fused(n, h, w, ci, co, dil, dtype, dispatch_cfg):
    """conv + bias + ReLU with the 2x2 max-pool in the epilogue == conv_igemm(EPI_BIAS_RELU) + max_pool2d, bitwise
    (both outputs; the 2-row pixel tiling must not change any conv value)."""
    from can_distributed_pytorch_amd.ops import conv as C
    dispatch_cfg(splitk=0)        # small grids: split-K sums k in another order than the unsplit kernels
    torch.manual_seed(12)
    x = torch.randn(n, h, w, ci, device="cuda").to(dtype)
    wt = torch.randn(co, ci, 3, 3, device="cuda") * (2.0 / (9 * ci)) ** 0.5
    b = torch.randn(co, device="cuda") * 0.1
    wp = C.pack_weight_fwd(wt, dtype)
    assert C.conv_pool_fwd_ok(x, co, 3)
    y, yp, codes = C.conv_pool_fwd(x, wp, b, ksize=3, dil=dil, codes=True)
    _, yp2, codes2 = C.conv_pool_fwd(x, wp, b, ksize=3, dil=dil, keep_full=False, codes=True)
    y_ref = C.conv_igemm(x, wp, b, ksize=3, dil=dil)
    yp_ref = F.max_pool2d(y_ref.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
    yp_ref2, codes_ref = C.maxpool_codes(y_ref)
    torch.cuda.synchronize()
    assert torch.equal(y, y_ref)
    assert torch.equal(yp, yp_ref) and torch.equal(yp_ref2, yp_ref)
    assert torch.equal(codes, codes_ref)
    assert torch.equal(yp2, yp) and torch.equal(codes2, codes)       # without the full-resolution store
    assert not C.conv_pool_fwd_ok(x[:, :h - 1].contiguous(), co, 3)     # odd H: not covered
    if ci == 64 and co == 64:                                            # halo kernel: whole 4-row tiles
        assert not C.conv_pool_fwd_ok(x[:, :h - 2].contiguous(), co, 3)
        assert not C.conv_pool_fwd_ok(x[:, :, :w - 32].contiguous(), co, 3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w,ci,co,tile", [(2, 8, 256, 128, 128, 29), (1, 6, 128, 256, 256, 27),
                                              (2, 4, 384, 64, 128, 29), (1, 10, 256, 128, 256, 0),
                                              (2, 6, 256, 128, 128, 0)])
def test_conv_pool_fwd_rring(n, h, w, ci, co, tile, dtype, dispatch_cfg):
    """Row-ring conv with the max-pool in the epilogue (2-row tiles, both rows per wave; tile 0 = dispatch
    rring_pool) == conv_igemm(EPI_BIAS_RELU) + max-pool codes, bitwise, with and without the full-size store."""
    from can_distributed_pytorch_amd.ops import conv as C
    dispatch_cfg(rring_pool=1, splitk=0)      # split-K (small grids) sums k in another order than cfg 21 / 22
    torch.manual_seed(13)
    x = torch.randn(n, h, w, ci, device="cuda").to(dtype)
    wt = torch.randn(co, ci, 3, 3, device="cuda") * (2.0 / (9 * ci)) ** 0.5
    b = torch.randn(co, device="cuda") * 0.1
    wp = C.pack_weight_fwd(wt, dtype)
    assert C.conv_pool_fwd_ok(x, co, 3, tile)
    y, yp, codes = C.conv_pool_fwd(x, wp, b, ksize=3, tile=tile, codes=True)
    _, yp2, codes2 = C.conv_pool_fwd(x, wp, b, ksize=3, tile=tile, keep_full=False, codes=True)
    y_ref = C.conv_igemm(x, wp, b, ksize=3)
    yp_ref, codes_ref = C.maxpool_codes(y_ref)
    torch.cuda.synchronize()
    assert torch.equal(y, y_ref)
    assert torch.equal(yp, yp_ref) and torch.equal(codes, codes_ref)
    assert torch.equal(yp2, yp) and torch.equal(codes2, codes)
    assert torch.equal(yp_ref, F.max_pool2d(y_ref.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))


@pytest.mark.parametrize("n,h,w,ci,co,dil,beta", [(2, 8, 64, 512, 256, 2, 0.0), (1, 6, 128, 1024, 512, 1, 1.0),
                                                    (2, 5, 64, 256, 512, 2, 0.5)])
def test_wgrad_tiled_reduction(n, h, w, ci, co, dil, beta):
    """The LDS-transposing slab reduction (coalesced dW writes) == the fp32 reference, beta and scale included."""
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(11)
    x = torch.randn(n, h, w, ci, device="cuda").to(torch.bfloat16)
    dy = torch.randn(n, h, w, co, device="cuda").to(torch.bfloat16)
    dw0 = torch.randn(co, ci, 3, 3, device="cuda")
    db0 = torch.randn(co, device="cuda")
    dw, db = dw0.clone(), db0.clone()
    C.conv_wgrad(dy, x, dw, db, ksize=3, dil=dil, beta=beta, scale=0.25)
    torch.cuda.synchronize()
    wr = torch.zeros(co, ci, 3, 3, device="cuda", requires_grad=True)
    br = torch.zeros(co, device="cuda", requires_grad=True)
    y = F.conv2d(x.float().permute(0, 3, 1, 2), wr, br, padding=dil, dilation=dil)
    gw, gb = torch.autograd.grad(y, (wr, br), dy.float().permute(0, 3, 1, 2))
    _close(dw, beta * dw0 + 0.25 * gw)
    _close(db, beta * db0 + 0.25 * gb)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w,ci,co", [(2, 12, 20, 128, 64), (1, 9, 13, 256, 128), (2, 6, 8, 512, 256),
                                         # row-ring data gradients (cfg 28 / 29 / 27: conv2_1 / conv3_1 / conv4_1)
                                         (2, 8, 128, 128, 64), (1, 6, 128, 256, 128), (1, 6, 256, 512, 256)])
def test_conv_dgrad_pool_backward_fused(n, h, w, ci, co, dtype):
    """EPI_POOLBWD (dgrad + max-pool backward + ReLU mask in one epilogue, driven by the max-pool codes) ==
    EPI_NONE + maxpool_bwd_codes == EPI_NONE + maxpool_bwd_relu on the pool input itself, bitwise."""
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(9)
    wt = (torch.randn(ci, co, 3, 3, device="cuda") * 0.05).to(dtype).float()   # layer co -> ci (dgrad maps ci -> co)
    dy = torch.randn(n, h, w, ci, device="cuda").to(dtype)
    full = torch.relu(torch.randn(n, 2 * h, 2 * w, co, device="cuda")).to(dtype)
    full[:, ::3, ::2] = 0                                          # ties and all-zero windows
    _, codes = C.maxpool_codes(full)
    pack = C.pack_weight_dgrad(wt, dtype)
    fused = C.conv_igemm(dy, pack, None, ksize=3, epi=C.EPI_POOLBWD, mask=codes)
    dp = C.conv_igemm(dy, pack, None, ksize=3, epi=C.EPI_NONE)
    via_codes = C.maxpool_bwd_codes(codes, dp)
    ref = torch.empty_like(full)
    _ext.require().maxpool_bwd_relu(full.data_ptr(), dp.data_ptr(), ref.data_ptr(), n, 2 * h, 2 * w, co,
                                    C.dt_code(dtype), _ext.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(via_codes, ref)
    assert torch.equal(fused, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w,ci,co,dil,epi", [
    (2, 12, 20, 128, 64, 1, "pool"), (1, 9, 13, 256, 128, 1, "pool"), (2, 6, 64, 512, 256, 1, "pool"),
    (2, 16, 96, 64, 64, 1, "mask"), (1, 10, 70, 128, 64, 1, "mask"), (2, 12, 128, 128, 128, 1, "mask"),
    (2, 8, 64, 512, 512, 2, "mask"), (1, 5, 40, 256, 128, 2, "mask"), (2, 8, 128, 64, 128, 1, "mask"),
    # > 512 partial rows: folded by the short launch conv_wgrad queues after its GEMM
    (8, 96, 128, 256, 512, 2, "mask"), (4, 48, 128, 128, 256, 1, "pool")])
def test_dgrad_bias_partials_feed_wgrad(n, h, w, ci, co, dil, epi, dtype):
    """The data-gradient epilogue's bias partials (EPI_MASK on the LDS-DMA and halo kernels, EPI_POOLBWD through
    the max-pool codes) reduce to the bias gradient of the tensor it writes: db from the partials == db from
    re-reading dY (bias_colsum / in-GEMM), and dW is untouched by the switch.  Here the conv maps co -> ci
    (dgrad of a ci -> co layer), so dX has ci channels."""
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(21)
    wt = (torch.randn(co, ci, 3, 3, device="cuda") * 0.05).to(dtype).float()   # layer ci -> co
    pack = C.pack_weight_dgrad(wt, dtype)                                         # dgrad: co -> ci
    dy = torch.randn(n, h, w, co, device="cuda").to(dtype)
    if epi == "pool":
        full = torch.relu(torch.randn(n, 2 * h, 2 * w, ci, device="cuda")).to(dtype)
        _, mask = C.maxpool_codes(full)
        e = C.EPI_POOLBWD
    else:
        mask = torch.randn(n, h, w, ci, device="cuda").to(dtype)
        e = C.EPI_MASK
    dx, bp = C.conv_dgrad_with_bias(dy, pack, ksize=3, dil=dil, epi=e, mask=mask)
    dx_plain = C.conv_igemm(dy, pack, None, ksize=3, dil=dil, epi=e, mask=mask)
    assert bp is not None and bp.shape[1] == ci
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_plain)                       # the partials do not change the written gradient
    # dX is the dY of the previous layer (ci channels): its weight gradient against some input
    xin = torch.randn(*dx.shape[:3], 64, device="cuda").to(dtype)
    dw1, db1 = torch.empty(ci, 64, 3, 3, device="cuda"), torch.empty(ci, device="cuda")
    dw2, db2 = torch.empty_like(dw1), torch.empty_like(db1)
    C.conv_wgrad(dx, xin, dw1, db1, ksize=3)
    C.conv_wgrad(dx, xin, dw2, db2, ksize=3, bias_partials=bp)
    torch.cuda.synchronize()
    assert torch.equal(dw1, dw2)
    ref = dx.float().sum(dim=(0, 1, 2))
    # partials sum the unrounded fp32 values: equal to the rounded-dY column sums to rounding
    assert torch.allclose(db2, ref, rtol=2e-2, atol=2e-2 * ref.abs().mean().item())
    assert torch.allclose(db1, ref, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("epi", ["fwd", "bias", "none", "dgrad", "pool"])
@pytest.mark.parametrize("n,h,w", [(2, 64, 640), (1, 61, 600), (3, 8, 1024), (1, 4, 64)])
def test_ws64_matches_halo_kernel(n, h, w, epi, dispatch_cfg):
    """Cin = Cout = 64 convs: the weight-stationary persistent kernel (several tiles per block, ragged tiles)
    == the per-tile halo kernel (ws64 = 0) bitwise — the same MFMA k order per output — and both == the
    fp32 reference."""
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(13)
    dev = "cuda"
    x = torch.randn(n, h, w, 64, device=dev).to(torch.bfloat16)
    wt = (torch.randn(64, 64, 3, 3, device=dev) * 0.05).to(torch.bfloat16).float()
    b = torch.randn(64, device=dev)
    mask = torch.randn(n, h, w, 64, device=dev).to(torch.bfloat16)
    if epi == "pool" and (h % 4 or w % 64):
        pytest.skip("fused pool: whole 4 x 64 tiles only")

    def run():
        if epi == "fwd":
            return (C.conv_igemm(x, C.pack_weight_fwd(wt), b, ksize=3),)
        if epi == "bias":
            return (C.conv_igemm(x, C.pack_weight_fwd(wt), b, ksize=3, epi=C.EPI_BIAS),)
        if epi == "none":
            return (C.conv_igemm(x, C.pack_weight_fwd(wt), None, ksize=3, epi=C.EPI_NONE),)
        if epi == "dgrad":
            return (C.conv_igemm(x, C.pack_weight_dgrad(wt), None, ksize=3, epi=C.EPI_MASK, mask=mask),)
        y, yp, codes = C.conv_pool_fwd(x, C.pack_weight_fwd(wt), b, ksize=3, codes=True)
        return y, yp, codes

    dispatch_cfg(ws64=1)
    new = run()
    dispatch_cfg(ws64=0)
    old = run()
    torch.cuda.synchronize()
    for a_, b_ in zip(new, old):
        assert torch.equal(a_, b_)
    if epi in ("fwd", "pool"):
        _close(new[0], _ref(x, wt, b, 1))
    elif epi == "dgrad":
        xr = torch.zeros(n, 64, h, w, device=dev, requires_grad=True)
        (gx,) = torch.autograd.grad(F.conv2d(xr, wt, None, padding=1), xr, x.float().permute(0, 3, 1, 2))
        _close(new[0], gx.permute(0, 2, 3, 1) * (mask.float() > 0))


@pytest.mark.parametrize("epi", [2, 4])
@pytest.mark.parametrize("n,h,w,ci,co,k", [(2, 12, 16, 512, 512, 1), (1, 9, 13, 128, 256, 3)])
def test_conv_igemm_batched_matches_per_item(n, h, w, ci, co, k, epi, dispatch_cfg):
    """nb convs in one launch (grid.y = item) == nb single launches, bitwise (context module conv{S}_2)."""
    from can_distributed_pytorch_amd.ops import conv as C
    dispatch_cfg(splitk=0)        # a small single launch would split K (the batched launch never does)
    torch.manual_seed(15)
    nb = 4
    x = torch.randn(nb, n, h, w, ci, device="cuda").to(torch.bfloat16)
    wp = torch.stack([C.pack_weight_fwd(torch.randn(co, ci, k, k, device="cuda") * 0.05) for _ in range(nb)])
    y = C.conv_igemm_batched(x, wp, ksize=k, epi=epi)
    ref = torch.stack([C.conv_igemm(x[i], wp[i], None, ksize=k, epi=epi) for i in range(nb)])
    torch.cuda.synchronize()
    assert torch.equal(y, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w,beta", [(2, 40, 128, 0.0), (1, 37, 150, 0.0), (2, 13, 70, 1.0), (1, 256, 512, 0.0)])
def test_conv_dgrad_w1g_fused(n, h, w, beta, dtype):
    """conv1_2's data gradient with conv1_1's weight gradient fused (ws64 W1G): dX bitwise equal to the plain ws64
    data gradient; dW1 / db1 vs fp32 PyTorch of conv1_1's weight gradient from that dX (ragged tiles, beta)."""
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(11)
    dev = "cuda"
    wt = (torch.randn(64, 64, 3, 3, device=dev) * 0.05).to(dtype).float()
    dgr = C.pack_weight_dgrad(wt, dtype)
    dy = torch.randn(n, h, w, 64, device=dev).to(dtype)
    mask = torch.randn(n, h, w, 64, device=dev).to(dtype)
    img = torch.randn(n, 3, h, w, device=dev)
    x4 = C.to_nhwc4(img, dtype)
    dx_ref = C.conv_igemm(dy, dgr, None, ksize=3, epi=C.EPI_MASK, mask=mask)
    cap = C.w1g_slab_cap(dev)
    sl = torch.full((cap, 36 * 64), float("nan"), device=dev)
    bsl = torch.full((cap, 64), float("nan"), device=dev)
    dw0 = torch.randn(64, 3, 3, 3, device=dev)
    db0 = torch.randn(64, device=dev)
    dw, db = dw0.clone(), db0.clone()
    dx = C.conv_dgrad_w1g(dy, dgr, mask, x4, dw, db, slabs=sl, bslabs=bsl, store_dx=True, beta=beta)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_ref)
    wr = torch.zeros(64, 3, 3, 3, device=dev, requires_grad=True)
    br = torch.zeros(64, device=dev, requires_grad=True)
    y = F.conv2d(x4[..., :3].float().permute(0, 3, 1, 2), wr, br, padding=1)
    gw, gb = torch.autograd.grad(y, (wr, br), dx_ref.float().permute(0, 3, 1, 2))
    _close(dw, gw + beta * dw0)
    _close(db, gb + beta * db0)
    # against the unfused first-layer weight gradient of the same dX
    dw2, db2 = dw0.clone(), db0.clone()
    C.conv_wgrad(dx_ref, x4, dw2, db2, ksize=3, first=True, beta=beta)
    _close(dw, dw2)
    _close(db, db2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w,ci,co,dil", [(2, 8, 128, 256, 256, 1), (1, 12, 128, 1024, 512, 2),
                                             (1, 6, 256, 128, 256, 1), (2, 10, 384, 64, 256, 2),
                                             (1, 4, 256, 512, 512, 2), (1, 2, 128, 192, 256, 1),
                                             # cfg 28: 64-channel 4-row tiles (8 row slots, 2-stage lead)
                                             (2, 8, 128, 128, 64, 1), (1, 8, 512, 128, 64, 1), (1, 4, 256, 256, 64, 2),
                                             # cfg 29: 128-channel 2-row tiles (the wave tile of cfg 22)
                                             (2, 6, 128, 256, 128, 1), (1, 4, 256, 384, 128, 2),
                                             # ragged: masked last column block (W % 128 != 0) / tile row (odd H)
                                             (2, 9, 240, 256, 256, 1), (1, 7, 200, 512, 512, 2),
                                             (1, 10, 240, 128, 64, 1), (2, 9, 120, 256, 128, 1),
                                             (1, 5, 480, 256, 256, 2), (1, 3, 104, 64, 64, 2)])
def test_row_ring_conv_bitwise(n, h, w, ci, co, dil, dtype, dispatch_cfg):
    """Row-ring 3x3 conv (cfg 27 / 28: activation rows staged once per 64-channel chunk, taps read shifted windows
    of the row slots) == the LDS-DMA kernel of the same tile (cfg 21 256 x 256 / cfg 23 64 x 512, rring = 0)
    bitwise for every epilogue it takes:
    bias + ReLU, plain, bias, ReLU-mask data gradient with bias partials, pool-backward data gradient, fp32 store;
    one- and multi-block-wide maps (zero guards / neighbour-pixel guards), dilation 1 and 2, top/bottom padding."""
    from can_distributed_pytorch_amd.ops import conv as C
    from can_distributed_pytorch_amd.ops import _ext
    torch.manual_seed(37)
    x = torch.randn(n, h, w, ci, device="cuda").to(dtype)
    wt = (torch.randn(co, ci, 3, 3, device="cuda") * (2.0 / (9 * ci)) ** 0.5).to(dtype).float()
    b = torch.randn(co, device="cuda") * 0.1
    wf = C.pack_weight_fwd(wt, dtype)
    wdt = (torch.randn(ci, co, 3, 3, device="cuda") * 0.05).to(dtype).float()     # a co -> ci layer: dgrad ci -> co
    wd = C.pack_weight_dgrad(wdt, dtype)
    mask = torch.randn(n, h, w, co, device="cuda").to(dtype)
    full = torch.relu(torch.randn(n, 2 * h, 2 * w, co, device="cuda")).to(dtype)
    full[:, ::3, ::2] = 0
    _, codes = C.maxpool_codes(full)
    ext = _ext.require()

    def run():
        r = [C.conv_igemm(x, wf, b, ksize=3, dil=dil),
             C.conv_igemm(x, wf, None, ksize=3, dil=dil, epi=C.EPI_NONE),
             C.conv_igemm(x, wf, b, ksize=3, dil=dil, epi=C.EPI_BIAS)]
        r += list(C.conv_dgrad_with_bias(x, wd, ksize=3, dil=dil, epi=C.EPI_MASK, mask=mask))
        r += list(C.conv_dgrad_with_bias(x, wd, ksize=3, dil=dil, epi=C.EPI_POOLBWD, mask=codes))
        y32 = torch.empty(n, h, w, co, dtype=torch.float32, device="cuda")
        ext.conv_igemm(x.data_ptr(), wf.data_ptr(), b.data_ptr(), 0, y32.data_ptr(), n, h, w, ci, co, 3, dil, 7, 0, 0,
                       C.dt_code(dtype), _ext.stream_ptr(x.device), 0, 0)
        r.append(y32)
        torch.cuda.synchronize()
        return r

    dispatch_cfg(rring=0, splitk=0)
    ref = run()
    # every dilation, 64-channel 4-row and 128-channel 2-row tiles; no split-K (its own test: a different k order)
    dispatch_cfg(rring=2, rring128=3, splitk=0)
    assert ext.conv_plan(h, w, ci, co, 3, dil, C.EPI_BIAS_RELU) in (27, 28, 29)    # the row ring really runs
    got = run()
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g is not None
        if i in (4, 6) and (w > 128 or h % (4 if co == 64 else 2)):
            # bias partials: one row per (tile, wave row); a multi-block-wide map groups the pixels of a row-ring
            # tile (2 rows x 128 columns) differently from a 256-pixel run, so only the column sums agree
            torch.testing.assert_close(g.sum(0), r.sum(0), rtol=1e-4, atol=1e-3)
        else:
            assert torch.equal(g, r), f"output {i} differs"
    # and against the fp32 reference (the cfg-21 path is covered there already; one direct check here)
    yref = torch.relu(torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), wt, b, padding=dil,
                                                 dilation=dil)).permute(0, 2, 3, 1)
    check_out16(got[0], yref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w,ci,co,dil", [(1, 96, 128, 512, 512, 2),     # backend at 1/8 of 768 x 1024, batch 1
                                             (1, 96, 128, 256, 512, 1),     # conv4_1
                                             (1, 85, 120, 512, 256, 2),     # ragged last tile row / column block
                                             (1, 48, 128, 512, 128, 1),     # cfg 29 (128-channel tiles)
                                             (2, 6, 256, 1024, 256, 1),
                                             (1, 60, 80, 512, 512, 2),      # 480 x 640 at 1/8 (one ragged block)
                                             (1, 120, 160, 256, 256, 1)])   # 480 x 640 at 1/4 (W % 128 != 0)
def test_row_ring_splitk(n, h, w, ci, co, dil, dtype, dispatch_cfg):
    """Row-ring split-K (_splitk_check)."""
    _splitk_check(n, h, w, ci, co, dil, dtype, dispatch_cfg, (27, 29))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w,ci,co,dil", [(1, 60, 72, 512, 512, 2),      # W = 72: no row ring (56 % of a block)
                                             (1, 120, 144, 256, 256, 1),    # W = 144: 56 % of two blocks
                                             (1, 30, 40, 512, 256, 2),
                                             (1, 60, 72, 256, 128, 1)])     # 128-channel tile
def test_glds_splitk(n, h, w, ci, co, dil, dtype, dispatch_cfg):
    """LDS-DMA v2 split-K (_splitk_check)."""
    _splitk_check(n, h, w, ci, co, dil, dtype, dispatch_cfg, (21, 22, 23, 25))


def test_splitk_concurrent_streams(dispatch_cfg):
    """Split-K scratch is per (device, launch stream) (conv_igemm.hip splitk_scratch): two split-K launches running
    at the same time on two streams (row ring and LDS-DMA v2) each use their own partials and arrival counters, so
    both equal their serial results bitwise, each stream holds its own slot and every counter is left at zero."""
    from can_distributed_pytorch_amd.ops import conv as C
    from can_distributed_pytorch_amd.ops import _ext
    torch.manual_seed(43)
    ext = _ext.require()
    dispatch_cfg(splitk=1)
    shapes = [(1, 96, 128, 512, 512, 2), (1, 60, 72, 512, 512, 2)]
    ops = []
    for n, h, w, ci, co, dil in shapes:
        assert ext.splitk_plan(n, h, w, ci, co, 3, dil, C.EPI_BIAS_RELU) > 1
        x = torch.randn(n, h, w, ci, device="cuda").to(torch.bfloat16)
        wt = (torch.randn(co, ci, 3, 3, device="cuda") * (2.0 / (9 * ci)) ** 0.5).to(torch.bfloat16).float()
        ops.append((x, C.pack_weight_fwd(wt, torch.bfloat16), torch.randn(co, device="cuda") * 0.1, dil))
    serial = [[C.conv_igemm(x, wf, b, ksize=3, dil=dil) for x, wf, b, dil in ops] for _ in range(2)]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    outs = [[], []]
    for _ in range(4):                                    # interleaved launches: the grids overlap on the device
        for k, s in enumerate((s1, s2)):
            with torch.cuda.stream(s):
                outs[k].append([C.conv_igemm(x, wf, b, ksize=3, dil=dil) for x, wf, b, dil in ops])
    torch.cuda.synchronize()
    for k in range(2):
        for rep in outs[k]:
            for got, ref in zip(rep, serial[0]):
                assert torch.equal(got, ref)
    assert ext.splitk_slots_used() >= 3                  # the default stream, s1, s2
    assert ext.splitk_dirty() == 0


def _splitk_check(n, h, w, ci, co, dil, dtype, dispatch_cfg, cfgs):
    """Split-K on a small grid (the input chunks split over KS blocks per tile, the last block to arrive sums the
    fp32 partials in part order and runs the epilogue): every epilogue (bias + ReLU, bias partials of the ReLU-mask
    data gradient, pool backward, fp32 store, fused pool) within the unsplit kernel's own error of the fp32
    reference, bias partials' column sums equal, and bitwise run-to-run (arrival order does not change the sum)."""
    from can_distributed_pytorch_amd.ops import conv as C
    from can_distributed_pytorch_amd.ops import _ext
    torch.manual_seed(41)
    ext = _ext.require()
    x = torch.randn(n, h, w, ci, device="cuda").to(dtype)
    wt = (torch.randn(co, ci, 3, 3, device="cuda") * (2.0 / (9 * ci)) ** 0.5).to(dtype).float()
    b = torch.randn(co, device="cuda") * 0.1
    wf = C.pack_weight_fwd(wt, dtype)
    wdt = (torch.randn(ci, co, 3, 3, device="cuda") * (1.0 / (9 * ci)) ** 0.5).to(dtype).float()
    wd = C.pack_weight_dgrad(wdt, dtype)
    mask = torch.randn(n, h, w, co, device="cuda").to(dtype)
    full = torch.relu(torch.randn(n, 2 * h, 2 * w, co, device="cuda")).to(dtype)
    _, codes = C.maxpool_codes(full)

    def run():
        y = C.conv_igemm(x, wf, b, ksize=3, dil=dil)
        dxm, bpm = C.conv_dgrad_with_bias(x, wd, ksize=3, dil=dil, epi=C.EPI_MASK, mask=mask)
        dxp, bpp = C.conv_dgrad_with_bias(x, wd, ksize=3, dil=dil, epi=C.EPI_POOLBWD, mask=codes)
        y32 = torch.empty(n, h, w, co, dtype=torch.float32, device="cuda")
        ext.conv_igemm(x.data_ptr(), wf.data_ptr(), b.data_ptr(), 0, y32.data_ptr(), n, h, w, ci, co, 3, dil, 7, 0, 0,
                       C.dt_code(dtype), _ext.stream_ptr(x.device), 0, 0)
        # the fused pool epilogue splits the same way (the row ring: 2-row tiles of an aligned map)
        pooled = None
        if dil == 1 and h % 2 == 0 and C.conv_pool_fwd_ok(x, co, 3):
            _, pooled, _ = C.conv_pool_fwd(x, wf, b, ksize=3, keep_full=False, codes=True)
        torch.cuda.synchronize()
        return [y, dxm, bpm.sum(0), dxp, bpp.sum(0), y32, pooled]

    dispatch_cfg(splitk=0)
    assert ext.splitk_plan(n, h, w, ci, co, 3, dil, C.EPI_BIAS_RELU) == 1
    one = run()
    dispatch_cfg(splitk=1)
    ks = ext.splitk_plan(n, h, w, ci, co, 3, dil, C.EPI_BIAS_RELU)
    assert ext.conv_plan(h, w, ci, co, 3, dil, C.EPI_BIAS_RELU) in cfgs and ks > 1, ks
    got = run()
    again = run()
    for i, (g, a) in enumerate(zip(got, again)):
        assert (g is None and a is None) or torch.equal(g, a), f"output {i} not repeatable"
    # fp32 references of the forward and the two data gradients
    xf = x.float().permute(0, 3, 1, 2)
    y32 = torch.nn.functional.conv2d(xf, wt, b, padding=dil, dilation=dil).permute(0, 2, 3, 1)
    d32 = torch.nn.functional.conv2d(xf, wdt.transpose(0, 1).flip(2, 3), None, padding=dil,
                                     dilation=dil).permute(0, 2, 3, 1)
    dm32 = d32 * (mask.float() > 0)
    # max-pool backward in fp32: code nibble of channel c (word c / 8, nibble c % 8), bit p = window position p
    nib = ((codes.unsqueeze(-1) >> (4 * torch.arange(8, device="cuda", dtype=torch.int32))) & 0xF).reshape(n, h, w, co)
    dp32 = torch.zeros(n, 2 * h, 2 * w, co, device="cuda")
    for p in range(4):
        dp32[:, p // 2::2, p % 2::2] = d32 * ((nib >> p) & 1).float()

    def err(a, r):
        return ((a.float() - r).norm() / (r.norm() + 1e-12)).item()
    refs = [(0, torch.relu(y32)), (1, dm32), (3, dp32), (5, y32)]
    if got[6] is not None:
        refs.append((6, torch.nn.functional.max_pool2d(torch.relu(y32).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)))
    for i, r in refs:
        e_split, e_one = err(got[i], r), err(one[i], r)
        assert e_split <= 1.05 * e_one + 1e-6, (i, e_split, e_one)
    torch.testing.assert_close(got[2], one[2], rtol=1e-4, atol=1e-2)
    torch.testing.assert_close(got[4], one[4], rtol=1e-4, atol=1e-2)
    # the fp32 store: only the k summation order differs
    torch.testing.assert_close(got[5], one[5], rtol=1e-5, atol=1e-4)
    assert ext.splitk_dirty() == 0          # every launch's last part reset its tiles' arrival counters


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_image_chunked_launches(dtype, monkeypatch):
    """Batches beyond the 32-bit per-launch operand size run as consecutive launches over image chunks (forced
    here with a tiny limit): forward / data gradient / fused pool / context GEMMs bitwise equal to one launch,
    weight gradients accumulated over the chunks equal to the fp32 reference."""
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(31)
    n, h, w = 5, 16, 128
    x64 = torch.randn(n, h, w, 64, device="cuda").to(dtype)
    x256 = torch.randn(n, h, w, 256, device="cuda").to(dtype)
    w1 = (torch.randn(256, 64, 3, 3, device="cuda") * 0.05).to(dtype).float()
    w2 = (torch.randn(256, 256, 3, 3, device="cuda") * 0.03).to(dtype).float()
    b = torch.randn(256, device="cuda")
    mask = torch.randn(n, h, w, 64, device="cuda").to(dtype)

    def run():
        y = C.conv_igemm(x64, C.pack_weight_fwd(w1, dtype), b, ksize=3)
        dx, part = C.conv_dgrad_with_bias(x256, C.pack_weight_dgrad(w1, dtype), ksize=3, mask=mask)
        _, yp, cd = C.conv_pool_fwd(x256, C.pack_weight_fwd(w2, dtype), b, ksize=3, keep_full=False, codes=True)
        dw = torch.empty(256, 64, 3, 3, device="cuda")
        db = torch.empty(256, device="cuda")
        C.conv_wgrad(x256, x64, dw, db, ksize=3)
        torch.cuda.synchronize()
        return y, dx, None if part is None else part.sum(0), yp, cd, dw, db

    one = run()
    monkeypatch.setattr(C, "MAX_ELEMS_PER_LAUNCH", 2 * h * w * 256)     # 2 images per launch -> 3 launches
    assert len(C.image_chunks(n, h * w * 256)) == 3
    many = run()
    for i in (0, 1, 3, 4):
        assert torch.equal(one[i], many[i]), i
    if one[2] is not None:
        torch.testing.assert_close(many[2], one[2], rtol=1e-5, atol=1e-3)
    xr = x64.float().permute(0, 3, 1, 2)
    wr = torch.zeros(256, 64, 3, 3, device="cuda", requires_grad=True)
    br = torch.zeros(256, device="cuda", requires_grad=True)
    gw, gb = torch.autograd.grad(F.conv2d(xr, wr, br, padding=1), (wr, br), x256.float().permute(0, 3, 1, 2))
    _close(many[5], gw)
    _close(many[6], gb)


# ---------------------------------------------------------------------------------------------------------------------
# Sign-bit ReLU masks (conv_igemm.hip EPI_MASKB): producers write sign_bits_ref(output) exactly, consumers give the
# bitwise result of the 16-bit mask map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w", [(2, 40, 256), (1, 37, 150)])
def test_sign_bits_first_layer(n, h, w, dtype):
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(5)
    wt = torch.randn(64, 3, 3, 3, device="cuda") * 0.3
    b = torch.randn(64, device="cuda") * 0.1
    x4 = C.to_nhwc4(torch.randn(n, 3, h, w, device="cuda"), dtype)
    wp = C.pack_weight_first(wt, dtype)
    bits = torch.full((n, h, w, 8), 0xAA, dtype=torch.uint8, device="cuda")
    y = C.conv_igemm(x4, wp, b, ksize=3, first=True, mask_bits_out=bits)
    y_ref = C.conv_igemm(x4, wp, b, ksize=3, first=True)
    torch.cuda.synchronize()
    assert torch.equal(y, y_ref)
    assert torch.equal(bits, C.sign_bits_ref(y))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w", [(2, 24, 256), (1, 13, 200)])
def test_sign_bits_halo64_and_dgrad_consumer(n, h, w, dtype):
    """conv2_1-like forward (Cin 64 -> 128, halo kernel) writes its sign bits; conv2_2-like data gradient (128 -> 128,
    128 x 512 LDS-DMA tile) with those bits as its ReLU mask == the same data gradient with the 16-bit map, bitwise,
    bias partials included."""
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(6)
    x = torch.randn(n, h, w, 64, device="cuda").to(dtype)
    wt = torch.randn(128, 64, 3, 3, device="cuda") * 0.05
    b = torch.randn(128, device="cuda") * 0.1
    bits = torch.zeros(n, h, w, 16, dtype=torch.uint8, device="cuda")
    y = C.conv_igemm(x, C.pack_weight_fwd(wt, dtype), b, ksize=3, mask_bits_out=bits)
    torch.cuda.synchronize()
    assert torch.equal(bits, C.sign_bits_ref(y))
    assert C.mask_bits_ok(h, w, 128, 128)
    w2 = torch.randn(128, 128, 3, 3, device="cuda") * 0.05
    dgr = C.pack_weight_dgrad(w2, dtype)
    dy = torch.randn(n, h, w, 128, device="cuda").to(dtype)
    dx_ref, bp_ref = C.conv_dgrad_with_bias(dy, dgr, ksize=3, mask=y)
    dx, bp = C.conv_dgrad_with_bias(dy, dgr, ksize=3, mask=None, mask_bits=bits)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_ref)
    assert (bp is None) == (bp_ref is None)
    if bp is not None:
        assert torch.equal(bp, bp_ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,h,w", [(2, 40, 128), (1, 37, 150), (1, 256, 512)])
def test_sign_bits_w1g_consumer(n, h, w, dtype):
    """conv1_2's fused data gradient + conv1_1 weight gradient with conv1_1's output as sign bits == with the map."""
    from can_distributed_pytorch_amd.ops import conv as C
    torch.manual_seed(12)
    dev = "cuda"
    wt = (torch.randn(64, 64, 3, 3, device=dev) * 0.05).to(dtype).float()
    dgr = C.pack_weight_dgrad(wt, dtype)
    dy = torch.randn(n, h, w, 64, device=dev).to(dtype)
    mask = torch.randn(n, h, w, 64, device=dev).to(dtype)
    x4 = C.to_nhwc4(torch.randn(n, 3, h, w, device=dev), dtype)
    cap = C.w1g_slab_cap(dev)
    outs = []
    for use_bits in (False, True):
        sl = torch.full((cap, 36 * 64), float("nan"), device=dev)
        bsl = torch.full((cap, 64), float("nan"), device=dev)
        dw = torch.zeros(64, 3, 3, 3, device=dev)
        db = torch.zeros(64, device=dev)
        dx = C.conv_dgrad_w1g(dy, dgr, None if use_bits else mask, x4, dw, db, slabs=sl, bslabs=bsl, store_dx=True,
                              mask_bits=C.sign_bits_ref(mask) if use_bits else None)
        outs.append((dx, dw, db))
    torch.cuda.synchronize()
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)


def test_sign_masks_step_bitwise(dispatch_cfg):
    """The production step with sign-bit masks (dispatch sign_masks = 1, default) == without, bitwise, at a shape
    where both producers and consumers take the sign-bit path."""
    import copy
    from can_distributed_pytorch_amd.engine.native import NativeStepper
    from can_distributed_pytorch_amd.models import CANNet
    from can_distributed_pytorch_amd.data.synthetic import make_synthetic_batch
    torch.manual_seed(4)
    base = CANNet().cuda()
    img, gt = make_synthetic_batch(2, 128, 512, seed=4, device="cuda")
    grads = []
    for sm in (0, 1):
        dispatch_cfg(sign_masks=sm)
        st = NativeStepper("cuda", lr=1e-7, graph=False, model=copy.deepcopy(base))
        st._step_body(img, gt, update=False)
        torch.cuda.synchronize()
        grads.append(st.arena.grad.clone())
        if sm:
            sv_bits = st.ex.forward_features(st.ex._img(img), save=True)[1]["mbits"]
            assert sorted(sv_bits) == [0, 2], sorted(sv_bits)       # conv1_1 and conv2_1 outputs
    assert torch.equal(grads[0], grads[1])
