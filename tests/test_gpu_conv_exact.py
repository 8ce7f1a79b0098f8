"""Every conv path bit for bit: the implicit-GEMM forward / data-gradient kernels (csrc/conv_igemm.hip) and the weight
gradients (csrc/conv_wgrad.hip, wgrad_ring.inc, wgrad_tap.inc) against the exact fp64 references of
tests/conv_exact_reference.py, with operands that are small integers times a power of two.

Such operands make every product and every partial sum, in any order, exact in fp32 (the asserted
``exactness_bound < 2^24``), so the kernel's accumulator is the mathematical result whatever the MFMA grouping, split-K
part order, slab reduction order or wave layout.  A 16-bit output must be its single round-to-nearest-even
(``R.to16``), an fp32 output the value itself (``R.to32``); every comparison is ``torch.equal`` and no tolerance exists.
tests/test_conv_exact_reference_cpu.py holds the references to F.conv2d / autograd and shows that the operand ranges
used here give outputs that need rounding, exact ties included, in both element types.

Every test asserts the kernel configuration it means to test (explicit ``tile=``, ``conv_plan``, ``splitk_plan``,
``wgrad_plan``), as tests/test_gpu_conv.py does; variants are selected with the ``dispatch_cfg`` fixture only.
A ``pytest.skip`` in this file is a launcher's refusal of a degenerate map, recorded with its return code.
"""
import re

import pytest
import torch

import conv_exact_reference as R
from elementwise_reference import maxpool_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
DTYPES = [torch.bfloat16, torch.float16]
BASIC = ("bias_relu", "bias", "none", "mask")             # epilogues every forward / data-gradient kernel takes
V2 = BASIC + ("maskbits", "pool", "f32")                  # LDS-DMA v2 tiles
RING = BASIC + ("pool", "f32")                            # row ring
MASK_RANGE = (-2, 2, 0)                                   # ReLU-mask maps: negative, zero and positive values


def _mods():
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops import conv as C
    return C, _ext.require(), _ext


def _or_skip(fn):
    """Run a launch; a refusal -- a negative return code of the launcher, or the front end's ValueError for a shape
    the launcher does not take -- becomes a skip that carries it.  HIP errors (positive codes) are failures."""
    try:
        return fn()
    except ValueError as e:
        pytest.skip(f"front end refused: {e}")
    except RuntimeError as e:
        if re.search(r"rc=-\d+", str(e)) is None:
            raise
        pytest.skip(f"launcher refused: {e}")


def _conv_operands(n, h, w, ci, co, k, dtype, seed, first=False):
    """x, the forward weight of a ci -> co layer with its bias, and the weight of a co -> ci layer whose data gradient
    maps x's ci channels to co (the same kernel with the flipped pack)."""
    o = {}
    if first:
        x16 = torch.zeros(n, h, w, 4, dtype=dtype, device=DEV)
        x16[..., :3] = R.int_operand((n, h, w, 3), R.X_FIRST, dtype, seed, DEV)[0]
        o["x16"], o["x"] = x16, x16.to(F64)
        o["w16"], o["w"] = R.int_operand((co, 3, 3, 3), R.W_FWD, dtype, seed + 1, DEV)
    else:
        o["x16"], o["x"] = R.int_operand((n, h, w, ci), R.X_ACT, dtype, seed, DEV)
        o["w16"], o["w"] = R.int_operand((co, ci, k, k), R.W_FWD, dtype, seed + 1, DEV)
        o["wd16"], o["wd"] = R.int_operand((ci, co, k, k), R.W_FWD, dtype, seed + 3, DEV)
    o["b32"], o["b"] = R.int_operand((co,), R.B_FWD, torch.float32, seed + 2, DEV)
    return o


def _check_conv(n, h, w, ci, co, k, dil, tile, dtype, epis, seed=100, first=False, launch=lambda fn: fn(), wvalid=None):
    """The epilogues ``epis`` of one kernel configuration against the exact references."""
    C, ext, _ext = _mods()
    o = _conv_operands(n, h, w, ci, co, k, dtype, seed, first)
    x16, x = o["x16"], o["x"]
    if wvalid is not None:                                 # a width-padded map: zero beyond the valid columns
        x16[:, :, wvalid:] = 0
        x = x16.to(F64)
    xr = R.first3(x) if first else x
    shift = R.W_FWD[2]
    assert R.exactness_bound(lambda a, c, d: R.conv_fwd_ref(a, c, d, dil, "bias"), (xr, o["w"], o["b"]), shift) < R.LIMIT
    wf = C.pack_weight_first(o["w16"].float(), dtype) if first else C.pack_weight_fwd(o["w16"].float(), dtype)
    y = R.conv_ref(xr, o["w"], dil)
    if wvalid is not None:
        y[:, :, wvalid:] = 0
    dt = C.dt_code(dtype)
    fwd = {"bias_relu": (C.EPI_BIAS_RELU, torch.relu(y + o["b"])), "bias": (C.EPI_BIAS, y + o["b"]),
           "none": (C.EPI_NONE, y)}
    if wvalid is not None:
        fwd["bias_relu"][1][:, :, wvalid:] = 0
        fwd["bias"][1][:, :, wvalid:] = 0
    d = None
    if any(e in ("mask", "maskbits", "pool") for e in epis):
        assert R.exactness_bound(lambda a, c: R.dgrad_ref(a, c, dil), (x, o["wd"]), shift) < R.LIMIT
        wd = C.pack_weight_dgrad(o["wd16"].float(), dtype)
        d = R.dgrad_ref(x, o["wd"], dil)
        mask16, mask = R.int_operand((n, h, w, co), MASK_RANGE, dtype, seed + 4, DEV)
    for e in epis:
        if e in fwd:
            code, ref = fwd[e]
            got = launch(lambda: C.conv_igemm(x16, wf, None if e == "none" else o["b32"], ksize=k, dil=dil, epi=code,
                                              first=first, tile=tile, wvalid=wvalid))
            want = R.to16(ref, dtype)
        elif e == "f32":
            got = torch.empty(n, h, w, co, dtype=torch.float32, device=DEV)
            launch(lambda: ext.conv_igemm(x16.data_ptr(), wf.data_ptr(), o["b32"].data_ptr(), 0, got.data_ptr(), n, h, w,
                                          ci, co, k, dil, 7, 0, tile, dt, _ext.stream_ptr(x16.device), 0, 0))
            want = R.to32(y + o["b"])
        elif e == "mask":
            got = launch(lambda: C.conv_igemm(x16, wd, None, ksize=k, dil=dil, epi=C.EPI_MASK, mask=mask16, tile=tile))
            want = R.to16(torch.where(mask > 0, d, torch.zeros_like(d)), dtype)
        elif e == "maskbits":
            bits = C.sign_bits_ref(mask16)
            got = launch(lambda: C.conv_igemm(x16, wd, None, ksize=k, dil=dil, epi=C.EPI_MASK, mask_bits=bits, tile=tile))
            want = R.to16(torch.where(mask > 0, d, torch.zeros_like(d)), dtype)
        elif e == "pool":
            full16, _ = R.relu_operand((n, 2 * h, 2 * w, co), R.POOL_MAP, dtype, seed + 5, DEV)
            _, codes, _ = maxpool_ref(full16)
            got = launch(lambda: C.conv_igemm(x16, wd, None, ksize=k, dil=dil, epi=C.EPI_POOLBWD, mask=codes, tile=tile))
            want = R.to16(R.poolbwd_ref(d, codes), dtype)
        else:
            raise AssertionError(e)
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"{e}: {int((got != want).sum())} of {want.numel()} elements differ"
    return o, y


# ---------------------------------------------------------------------------------------- forward and data gradient
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,ci,co,k,dil,tile", [
    # generic kernel, every tile
    (1, 20, 20, 128, 256, 3, 1, 1), (1, 20, 20, 128, 256, 3, 1, 2), (1, 20, 20, 128, 256, 3, 1, 3),
    (1, 20, 20, 128, 256, 3, 1, 4), (2, 9, 13, 64, 128, 3, 2, 1), (1, 9, 13, 128, 128, 1, 1, 2),
    # LDS-DMA v1 tiles
    (1, 20, 20, 128, 256, 3, 1, 11), (1, 20, 20, 128, 256, 3, 1, 12), (1, 20, 20, 128, 256, 3, 1, 13),
    (2, 9, 13, 64, 128, 3, 2, 12)])
def test_generic_and_v1_tiles(n, h, w, ci, co, k, dil, tile, dtype):
    _check_conv(n, h, w, ci, co, k, dil, tile, dtype, BASIC)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,ci,co,k,dil,tile", [
    (1, 20, 20, 128, 256, 3, 1, 21), (1, 20, 20, 128, 256, 3, 1, 22), (1, 20, 20, 128, 256, 3, 1, 23),
    (1, 20, 40, 128, 128, 3, 1, 25),
    # 1x1 (nk = Cin / 64, nk = 1), dilation 2 with a ragged last tile, the largest K of the model
    (1, 9, 13, 64, 256, 1, 1, 21), (1, 5, 7, 128, 384, 1, 1, 25), (2, 9, 13, 64, 128, 3, 2, 22),
    (3, 11, 17, 64, 64, 3, 1, 23), (2, 9, 13, 256, 128, 3, 2, 25), (1, 12, 16, 1024, 512, 3, 2, 21)])
def test_v2_tiles(n, h, w, ci, co, k, dil, tile, dtype, dispatch_cfg):
    dispatch_cfg(splitk=0)                                 # split-K has its own test
    _check_conv(n, h, w, ci, co, k, dil, tile, dtype, V2 if k == 3 else BASIC + ("f32",))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,co,ws64", [(2, 10, 200, 64, 0), (1, 9, 130, 128, 0), (2, 3, 7, 128, 0), (1, 4, 64, 64, 0),
                                           (2, 10, 200, 64, 1), (1, 4, 64, 64, 1), (1, 61, 600, 64, 1)])
def test_halo_and_ws64(n, h, w, co, ws64, dtype, dispatch_cfg):
    """Cin = 64 halo kernel (Cout 64 / 128) and, for Cout = 64, its weight-stationary persistent form (several tiles
    per block at the last shape)."""
    C, ext, _ = _mods()
    dispatch_cfg(ws64=ws64)
    assert ext.conv_plan(h, w, 64, co, 3, 1, C.EPI_BIAS_RELU) == (33 if (ws64 and co == 64) else 31)
    _check_conv(n, h, w, 64, co, 3, 1, 31, dtype, BASIC)
    _check_conv(n, h, w, 64, co, 3, 1, 0, dtype, ("bias_relu",), seed=7)       # the automatic choice is the same kernel


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,ci,co,dil,cfg", [
    (2, 8, 128, 256, 256, 1, 27), (2, 8, 128, 128, 64, 1, 28), (2, 6, 128, 256, 128, 1, 29),
    # ragged: masked last column block / tile row; dilation 2
    (2, 9, 240, 256, 256, 1, 27), (1, 3, 104, 64, 64, 2, 28), (1, 4, 256, 384, 128, 2, 29), (1, 10, 240, 128, 64, 1, 28)])
def test_row_ring(n, h, w, ci, co, dil, cfg, dtype, dispatch_cfg):
    C, ext, _ = _mods()
    dispatch_cfg(rring=2, rring128=3, splitk=0)
    for e in (C.EPI_BIAS_RELU, C.EPI_MASK, C.EPI_POOLBWD, 7):
        assert ext.conv_plan(h, w, ci, co, 3, dil, e) == cfg
    _check_conv(n, h, w, ci, co, 3, dil, 0, dtype, RING)
    _check_conv(n, h, w, ci, co, 3, dil, cfg, dtype, ("bias_relu", "mask"), seed=11)     # the explicit tile too


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,tile", [(2, 40, 56, 0), (1, 37, 150, 32), (2, 8, 256, 0), (2, 40, 56, 2),
                                        (1, 9, 13, 2)])
def test_first_layer(n, h, w, tile, dtype):
    """tile 0 / 32: the halo-tiled first-layer kernel (with the output's sign bits); 2: the generic kernel's 64-channel
    tile (the only one Cout = 64 fills)."""
    C, _, _ = _mods()
    o, y = _check_conv(n, h, w, 4, 64, 3, 1, tile, dtype, ("bias_relu",), first=True)
    if tile in (0, 32):
        bits = torch.full((n, h, w, 8), 0xAA, dtype=torch.uint8, device=DEV)
        got = C.conv_igemm(o["x16"], C.pack_weight_first(o["w16"].float(), dtype), o["b32"], ksize=3, first=True,
                           tile=tile, mask_bits_out=bits)
        want = R.to16(torch.relu(y + o["b"]), dtype)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        assert torch.equal(bits, C.sign_bits_ref(want))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w", [(2, 24, 256), (1, 13, 200)])
def test_sign_bits_out_halo(n, h, w, dtype):
    """The 64 -> 128 halo kernel writes the sign bits of its exact output."""
    C, _, _ = _mods()
    o = _conv_operands(n, h, w, 64, 128, 3, dtype, 21)
    assert R.exactness_bound(lambda a, c, d: R.conv_fwd_ref(a, c, d, 1, "bias"), (o["x"], o["w"], o["b"]), 6) < R.LIMIT
    bits = torch.full((n, h, w, 16), 0x55, dtype=torch.uint8, device=DEV)
    got = C.conv_igemm(o["x16"], C.pack_weight_fwd(o["w16"].float(), dtype), o["b32"], ksize=3, tile=31,
                       mask_bits_out=bits)
    want = R.to16(R.conv_fwd_ref(o["x"], o["w"], o["b"]), dtype)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(bits, C.sign_bits_ref(want))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,wv,ci,co,tile,first", [
    (2, 8, 128, 100, 128, 256, 21, False), (1, 9, 192, 130, 64, 128, 31, False), (2, 6, 256, 250, 256, 256, 27, False),
    (1, 10, 128, 77, 64, 64, 31, False), (2, 12, 256, 201, 4, 64, 0, True)])
def test_width_padded_maps(n, h, w, wv, ci, co, tile, first, dtype, dispatch_cfg):
    """wvalid: the first wv columns are the image, the rest zero padding that the forward epilogues write as zero."""
    dispatch_cfg(rring=2, splitk=0)
    _check_conv(n, h, w, ci, co, 3, 1, tile, dtype, ("bias_relu",) if first else ("bias_relu", "bias"), first=first,
                wvalid=wv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,ci,co,k,tile", [(2, 12, 16, 512, 512, 1, 0), (1, 9, 13, 128, 256, 3, 0),
                                                (1, 9, 13, 128, 128, 3, 22)])
def test_batched(n, h, w, ci, co, k, tile, dtype):
    """conv_igemm_batched, EPI_NONE: every item against its own exact reference."""
    C, _, _ = _mods()
    nb = 3
    items = [_conv_operands(n, h, w, ci, co, k, dtype, 30 + 10 * i) for i in range(nb)]
    x = torch.stack([o["x16"] for o in items])
    wp = torch.stack([C.pack_weight_fwd(o["w16"].float(), dtype) for o in items])
    for o in items:
        assert R.exactness_bound(lambda a, c: R.conv_ref(a, c, 1), (o["x"], o["w"]), 6) < R.LIMIT
    got = C.conv_igemm_batched(x, wp, ksize=k, epi=C.EPI_NONE, tile=tile)
    torch.cuda.synchronize()
    for i, o in enumerate(items):
        assert torch.equal(got[i], R.to16(R.conv_ref(o["x"], o["w"], 1), dtype)), i


# -------------------------------------------------------------------------------------------------- fused pool forward
def _check_pool_fwd(n, h, w, ci, co, dil, tile, dtype, seed=50):
    C, _, _ = _mods()
    o = _conv_operands(n, h, w, ci, co, 3, dtype, seed)
    assert R.exactness_bound(lambda a, c, d: R.conv_fwd_ref(a, c, d, dil, "bias"), (o["x"], o["w"], o["b"]), 6) < R.LIMIT
    wf = C.pack_weight_fwd(o["w16"].float(), dtype)
    assert C.conv_pool_fwd_ok(o["x16"], co, 3, tile)
    full, pooled, codes = R.pool_fwd_ref(o["x"], o["w"], o["b"], dtype, dil)
    y, yp, cd = C.conv_pool_fwd(o["x16"], wf, o["b32"], ksize=3, dil=dil, tile=tile, codes=True)
    y2, yp2, cd2 = C.conv_pool_fwd(o["x16"], wf, o["b32"], ksize=3, dil=dil, tile=tile, keep_full=False, codes=True)
    torch.cuda.synchronize()
    assert y2 is None
    assert torch.equal(y, full)
    assert torch.equal(yp, pooled) and torch.equal(cd, codes)
    assert torch.equal(yp2, pooled) and torch.equal(cd2, codes)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,ci,co,dil,cfg", [(1, 6, 256, 256, 256, 1, 21), (2, 4, 256, 256, 128, 2, 22),
                                                 (1, 4, 512, 128, 64, 1, 23), (2, 8, 512, 128, 128, 1, 25)])
def test_pool_fwd_v2(n, h, w, ci, co, dil, cfg, dtype, dispatch_cfg):
    C, ext, _ = _mods()
    dispatch_cfg(splitk=0, rring_pool=0)
    assert ext.conv_plan(h, w, ci, co, 3, dil, 6) == cfg   # EPI_POOLFWD: the config conv_pool_fwd launches
    _check_pool_fwd(n, h, w, ci, co, dil, 0, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws64", [1, 0])
@pytest.mark.parametrize("n,h,w", [(2, 8, 128), (1, 12, 320)])
def test_pool_fwd_halo(n, h, w, ws64, dtype, dispatch_cfg):
    C, ext, _ = _mods()
    dispatch_cfg(ws64=ws64)
    assert ext.conv_plan(h, w, 64, 64, 3, 1, C.EPI_BIAS_RELU) == (33 if ws64 else 31)
    _check_pool_fwd(n, h, w, 64, 64, 1, 0, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,ci,co,tile", [(2, 8, 256, 128, 128, 29), (1, 6, 128, 256, 256, 27),
                                              (2, 4, 384, 64, 128, 29)])
def test_pool_fwd_row_ring(n, h, w, ci, co, tile, dtype, dispatch_cfg):
    dispatch_cfg(rring_pool=1, splitk=0)
    _check_pool_fwd(n, h, w, ci, co, 1, tile, dtype)


# ------------------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,ci,co,dil,cfgs", [
    (2, 6, 256, 1024, 256, 1, (27,)), (1, 48, 128, 512, 128, 1, (29,)), (1, 60, 80, 512, 512, 2, (27,)),
    (1, 30, 40, 512, 256, 2, (21,)), (1, 60, 72, 256, 128, 1, (22,))])
def test_split_k(n, h, w, ci, co, dil, cfgs, dtype, dispatch_cfg):
    """Split-K (the input chunks of a tile over KS blocks, the last to arrive sums the fp32 partials): every element of
    every epilogue against the exact reference -- any part order sums these operands exactly -- and every arrival
    counter left at zero."""
    C, ext, _ = _mods()
    dispatch_cfg(splitk=1, rring=2, rring128=3)
    for e in (C.EPI_BIAS_RELU, C.EPI_MASK, C.EPI_POOLBWD, 7):
        assert ext.conv_plan(h, w, ci, co, 3, dil, e) in cfgs
        assert ext.splitk_plan(n, h, w, ci, co, 3, dil, e) > 1
    _check_conv(n, h, w, ci, co, 3, dil, 0, dtype, ("bias_relu", "mask", "pool", "f32"), seed=60)
    o = _conv_operands(n, h, w, ci, co, 3, dtype, 60)
    if dil == 1 and h % 2 == 0 and C.conv_pool_fwd_ok(o["x16"], co, 3):
        _check_pool_fwd(n, h, w, ci, co, 1, 0, dtype, seed=60)
    assert ext.splitk_dirty() == 0


# ------------------------------------------------------------------------------------------------------ bias partials
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,ci,co,dil,epi,splitk,many", [
    (2, 12, 20, 128, 64, 1, "pool", 0, False), (2, 16, 96, 64, 64, 1, "mask", 0, False),
    (1, 10, 70, 128, 64, 1, "mask", 0, False), (2, 8, 64, 512, 512, 2, "mask", 0, False),
    (2, 8, 128, 64, 128, 1, "mask", 0, False), (2, 6, 64, 512, 256, 1, "pool", 0, False),
    # the last-arriving split-K block writes the partials (LDS-DMA v2, row ring)
    (1, 30, 40, 256, 512, 2, "mask", 1, False), (2, 6, 256, 256, 1024, 1, "mask", 1, False),
    # more than 512 partial rows (the halo kernel: 4 per 4 x 64 tile): folded by conv_wgrad's short launch
    (129, 2, 4, 64, 64, 1, "mask", 0, True)])
def test_bias_partials(n, h, w, ci, co, dil, epi, splitk, many, dtype, dispatch_cfg):
    """The data-gradient epilogue's bias partials: their fp64 column sums equal the column sums of the UNROUNDED
    (masked / pool-routed) gradient exactly, and conv_wgrad(bias_partials=) gives that db exactly; without them db is
    the exact column sum of the rounded gradient.  The layer is ci -> co, so the data gradient maps co -> ci.
    Sparse operands (R.sparse_density) keep a whole channel's sum below 2^24 while the values still need rounding."""
    C, ext, _ = _mods()
    dispatch_cfg(splitk=splitk, ws64=1)
    M, K = n * h * w, 9 * co
    dens = R.sparse_density(K, M)
    dy16, dy = R.int_operand((n, h, w, co), R.X_ACT, dtype, 70, DEV, density=dens)
    w16, wt = R.int_operand((co, ci, 3, 3), R.W_BP, dtype, 71, DEV, density=dens)
    assert R.bias_partial_bound(lambda a, c: R.dgrad_ref(a, c, dil), (dy, wt), R.W_BP[2]) < R.LIMIT
    d = R.dgrad_ref(dy, wt, dil)
    if epi == "pool":
        full16, _ = R.relu_operand((n, 2 * h, 2 * w, ci), R.POOL_MAP, dtype, 72, DEV)
        _, mask, _ = maxpool_ref(full16)
        exact, e = R.poolbwd_ref(d, mask), C.EPI_POOLBWD
    else:
        mask, m64 = R.int_operand((n, h, w, ci), MASK_RANGE, dtype, 72, DEV)
        exact, e = torch.where(m64 > 0, d, torch.zeros_like(d)), C.EPI_MASK
    share, ties = R.rounding_stats(exact, dtype)
    assert share >= 0.01 and ties >= 8, (share, ties)     # summing the rounded values would give another db
    if splitk:
        assert ext.splitk_plan(n, h, w, co, ci, 3, dil, e) > 1
    pack = C.pack_weight_dgrad(w16.float(), dtype)
    dx, bp = C.conv_dgrad_with_bias(dy16, pack, ksize=3, dil=dil, epi=e, mask=mask)
    torch.cuda.synchronize()
    assert bp is not None and bp.shape[1] == ci
    assert (bp.shape[0] > C.BIAS_ROWS) == many
    rounded = R.to16(exact, dtype)
    assert torch.equal(dx, rounded)
    colsum = exact.reshape(-1, ci).sum(0)
    assert torch.equal(bp.double().sum(0), colsum)
    # dX is the dY of the previous layer: its bias gradient from the partials, and from re-reading the rounded dX
    colsum16 = rounded.to(F64).reshape(-1, ci).sum(0)
    assert float(rounded.to(F64).abs().reshape(-1, ci).sum(0).max()) * 2.0 ** R.W_BP[2] < R.LIMIT
    xin, _ = R.int_operand((*dx.shape[:3], 64), R.X_WG, dtype, 73, DEV)
    dw = torch.empty(ci, 64, 3, 3, device=DEV)
    db1, db2 = torch.full((ci,), float("nan"), device=DEV), torch.full((ci,), float("nan"), device=DEV)
    C.conv_wgrad(dx, xin, dw, db2, ksize=3, bias_partials=bp)
    C.conv_wgrad(dx, xin, dw, db1, ksize=3)
    torch.cuda.synchronize()
    assert torch.equal(db2, R.to32(colsum))
    assert torch.equal(db1, R.to32(colsum16))
    if splitk:
        assert ext.splitk_dirty() == 0


# ---------------------------------------------------------------------------------------------------- weight gradient
_RED_KIND = {"tiled": 0, "r1": 1, "r4": 4, "r16": 16, "r64": 64}     # the launch plan's "reduce" (wgrad_plan.h)
_WG_GLDS, _WG_GLDS2 = 1, 2                                            # ... and "family": the v1 / v2 LDS-DMA kernels


def _reduce_kernel(S, K, co, ci, taps, first):
    """The slab reduction conv_wgrad.hip launch_reduce2 picks: the LDS-transposing tiled kernel, or
    wgrad_reduce2_kernel<1 / 4 / 64 / 16>."""
    if not first and taps == 9 and S <= 16 and co % 64 == 0 and ci % 8 == 0 and (co // 64) * (ci // 8) >= 256:
        return "tiled"
    if S <= 16:
        return "r1"
    if S <= 128:
        return "r4"
    return "r64" if K * co < 4096 else "r16"


def _wg_ranges(M):
    """+-12 operands while M * 144 stays below 2^24, else +-3 (M up to 262144 * 9 / 9)."""
    return R.X_ACT if M * 144 < R.LIMIT else R.X_WG


def _check_wgrad(n, h, w, ci, co, k, dil, dtype, cfg, red=None, beta=0.0, scale=1.0, dscale_k=None, bias=True,
                 first=False, launch=lambda fn: fn(), seed=80):
    C, ext, _ = _mods()
    M = n * h * w
    rng = _wg_ranges(M)
    if first:
        x16 = torch.zeros(n, h, w, 4, dtype=dtype, device=DEV)
        x16[..., :3] = R.int_operand((n, h, w, 3), rng, dtype, seed, DEV)[0]
        x = R.first3(x16.to(F64))
    else:
        x16, x = R.int_operand((n, h, w, ci), rng, dtype, seed, DEV)
    dy16, dy = R.int_operand((n, h, w, co), rng, dtype, seed + 1, DEV)
    cw = 3 if first else ci
    dw0, dw064 = R.int_operand((co, cw, k, k), (-64, 64, 0), torch.float32, seed + 2, DEV)
    db0, db064 = R.int_operand((co,), (-64, 64, 0), torch.float32, seed + 3, DEV)
    ds = 1.0 if dscale_k is None else 2.0 ** -dscale_k
    # in units of scale * dscale (a power of two): the gradient's bound plus the beta * dw0 term
    assert R.exactness_bound(lambda a, c: R.wgrad_ref(a, c, k, dil), (dy, x), 0) + 64 / (scale * ds) < R.LIMIT
    gw, gb = R.wgrad_ref(dy, x, k, dil)
    ws = C.WgradWorkspace(DEV)
    s, _, got_cfg, _ = ws.plan(M, ci, co, k, first, dil, w)
    assert got_cfg == cfg, (got_cfg, s)
    plan = ext.wgrad_launch_plan(n, h, w, M, ci, co, k, dil, int(first), want_db=bias)
    if plan["err"]:
        assert plan["err"] == -3 and (h < 2 or w < 2), plan    # the launch below is refused with this code
    else:
        assert (plan["cfg"], plan["S"]) == (cfg, s), plan
    if red is not None:
        assert _reduce_kernel(s, 64 if first else k * k * ci, co, 4 if first else ci, k * k, first) == red, s
        assert plan["reduce"] == _RED_KIND[red], plan
    if cfg in (9, 10, 11) and not plan["err"]:
        # the kernel that runs: the pipelined v2 kernel on the 3x3 layers (row-aligned and ragged widths alike), the v1
        # kernel of the same tiles on a 1x1 layer whose width is no multiple of 64
        assert plan["family"] == (_WG_GLDS if k == 1 and w % 64 else _WG_GLDS2), plan
        assert plan["ragged"] == (k == 3 and w % 64 != 0), plan
    dw, db = dw0.clone(), (db0.clone() if bias else None)
    dsc = None if dscale_k is None else torch.tensor([ds], dtype=torch.float32, device=DEV)
    launch(lambda: C.conv_wgrad(dy16, x16, dw, db, ksize=k, dil=dil, first=first, ws=ws, beta=beta, scale=scale,
                                dscale=dsc))
    torch.cuda.synchronize()
    want = R.to32(R.wgrad_update_ref(gw, dw064, beta, scale, ds))
    assert torch.equal(dw, want), f"dw: {int((dw != want).sum())} of {want.numel()} elements differ"
    if bias:
        assert torch.equal(db, R.to32(R.wgrad_update_ref(gb, db064, beta, scale, ds)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,ci,co,k,dil,cfg,red", [
    (1, 6, 8, 64, 128, 3, 1, 1, "r1"), (1, 6, 8, 192, 256, 3, 1, 2, "r1"), (2, 13, 11, 64, 64, 3, 1, 3, "r1"),
    (1, 9, 13, 64, 64, 1, 1, 4, "r1"), (1, 7, 9, 320, 128, 3, 1, 6, "r1"), (1, 7, 9, 320, 256, 3, 2, 7, "r1"),
    (1, 48, 48, 64, 64, 3, 1, 3, "r4"), (2, 16, 24, 512, 512, 1, 1, 9, "r1"),       # 1x1, W % 64 != 0: cfg 7's tiles
    # v2 pipelined kernels, aligned and ragged widths
    (1, 6, 64, 256, 256, 3, 1, 9, None), (2, 7, 100, 256, 256, 3, 1, 9, "r4"), (2, 5, 64, 256, 512, 3, 2, 9, "tiled"),
    (1, 6, 64, 128, 256, 3, 1, 10, None), (1, 6, 90, 128, 256, 3, 1, 10, None), (2, 5, 128, 128, 512, 3, 2, 10, None),
    (1, 9, 64, 256, 128, 3, 2, 11, None), (2, 5, 100, 512, 128, 3, 2, 11, None)])
def test_wgrad_generic_and_v2(n, h, w, ci, co, k, dil, cfg, red, dtype, dispatch_cfg):
    dispatch_cfg(wgrad_tap=0)
    _check_wgrad(n, h, w, ci, co, k, dil, dtype, cfg, red)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,ci,co,dil", [
    (1, 6, 64, 64, 128, 1), (2, 7, 128, 128, 256, 1), (1, 9, 120, 256, 128, 2), (1, 1, 64, 64, 128, 1),
    (1, 3, 40, 64, 128, 2), (2, 9, 128, 1024, 512, 2),          # 4 slices over 36 stages: slices spanning chains
    # the 64-channel tile
    (1, 6, 64, 64, 64, 1), (2, 9, 120, 128, 64, 2), (1, 5, 200, 64, 64, 1), (3, 16, 256, 64, 64, 1)])
def test_wgrad_tap_ring(n, h, w, ci, co, dil, dtype, dispatch_cfg):
    dispatch_cfg(wgrad_tap=3)
    _check_wgrad(n, h, w, ci, co, 3, dil, dtype, 12)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,c,red", [
    (1, 257, 1021, 64, "r16"),        # general addressing: odd H, W % 64 != 0, the smallest such map over the threshold
    (2, 128, 1024, 128, "r4")])       # fast addressing at M = 262144 exactly: 2 images, 16 strips, 2 x 2 channel tiles
def test_wgrad_ring_at_threshold(n, h, w, c, red, dtype, dispatch_cfg):
    """cfg 8 (halo / ring weight gradient, M >= 262144): every element of dw is an exact integer, so one dropped,
    doubled or misplaced pixel changes it -- the arithmetic tests/test_gpu_conv.py cannot do at this M."""
    dispatch_cfg(wgrad_tap=0)
    assert n * h * w >= 262144 and n * h * w < 262144 * 1.001
    _check_wgrad(n, h, w, c, c, 3, 1, dtype, 8, red)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wgrad_first_layer(dtype):
    _check_wgrad(2, 40, 56, 4, 64, 3, 1, dtype, 0, "r4", first=True)
    _check_wgrad(1, 9, 13, 4, 64, 3, 1, dtype, 0, "r1", beta=1.0, scale=0.25, first=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,ci,co,dil,beta,dscale_k", [(2, 8, 64, 512, 256, 2, 0.0, 3), (1, 6, 128, 1024, 512, 1, 1.0, None),
                                                           (2, 5, 64, 256, 512, 2, 0.5, 10), (2, 13, 11, 64, 64, 1, 0.5, 1)])
def test_wgrad_beta_scale_dscale(n, h, w, ci, co, dil, beta, dscale_k, dtype, dispatch_cfg):
    """dw = beta dw0 + scale dscale sum: dw0 integers, scale 0.25 and the device scalar 2^-k keep every value exact.
    The first three run the LDS-transposing slab reduction, the last wgrad_reduce2_kernel<1>."""
    dispatch_cfg(wgrad_tap=0)
    small = ci == 64
    _check_wgrad(n, h, w, ci, co, 3, dil, dtype, 3 if small else 9, "r1" if small else "tiled", beta=beta, scale=0.25,
                 dscale_k=dscale_k)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,beta,scale,dscale_k", [(1, 3, 64, 0.0, 1.0, None), (2, 5, 67, 0.0, 1.0, None),
                                                       (2, 5, 67, 0.5, 0.25, 3)])
def test_wgrad_ctx_dw2cat_shape(n, h, w, beta, scale, dscale_k, dtype, dispatch_cfg):
    """The linearised context module's dW2cat launch (ops/context_exec.py ctx2_wgrad): 1x1, 512 -> 2048, no bias.
    wgrad_plan.h gives it cfg 9 by the "1x1 with many output rows" rule (K = 512 < 2048): 8 x 2 tiles of 256 x 256,
    at most 16 pixel slices of whole 64-pixel stages (3 slices at M = 192, 11 at M = 670), so wgrad_reduce2_kernel<1>
    sums the slabs; the v2 kernel at a width of 64, the v1 kernel of cfg 7's tiles at 67 (asserted by _check_wgrad)."""
    dispatch_cfg(wgrad_tap=0)
    _check_wgrad(n, h, w, 512, 2048, 1, 1, dtype, 9, "r1", beta=beta, scale=scale, dscale_k=dscale_k, bias=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wgrad_1x1_batched(dtype):
    C, _, _ = _mods()
    nb, n, h, w, c = 4, 2, 12, 128, 512
    dy16, dy = R.int_operand((nb, n, h, w, c), R.X_ACT, dtype, 90, DEV)
    x16, x = R.int_operand((nb, n, h, w, c), R.X_ACT, dtype, 91, DEV)
    assert n * h * w * 144 * 2 < R.LIMIT                   # scale 0.5: units of one half
    arena = torch.full((nb * c * c,), float("nan"), device=DEV)
    dws = [arena[i * c * c:(i + 1) * c * c].view(c, c, 1, 1) for i in range(nb)]
    assert C.wgrad_1x1_batched_ok(dy16, x16, dws)
    C.conv_wgrad_1x1_batched(dy16, x16, dws, ws=C.WgradWorkspace(DEV), scale=0.5)
    torch.cuda.synchronize()
    for b in range(nb):
        want = R.to32(0.5 * (dy[b].reshape(-1, c).t() @ x[b].reshape(-1, c)))
        assert torch.equal(dws[b].view(c, c), want), b


@pytest.mark.parametrize("dtype", DTYPES)
def test_image_chunks(dtype, monkeypatch, dispatch_cfg):
    """Batches beyond the per-launch operand size run as launches over image chunks: the forward bitwise, the weight
    gradient accumulated over the chunks (beta = 1 after the first) still the exact sum."""
    C, _, _ = _mods()
    n, h, w = 5, 16, 128
    dispatch_cfg(wgrad_tap=0)
    monkeypatch.setattr(C, "MAX_ELEMS_PER_LAUNCH", 2 * h * w * 256)     # 2 images per launch -> 3 launches
    assert len(C.image_chunks(n, h * w * 256)) == 3
    _check_wgrad(n, h, w, 64, 256, 3, 1, dtype, 1, beta=0.5)
    _check_conv(n, h, w, 64, 256, 3, 1, 0, dtype, ("bias_relu", "mask"))


# ------------------------------------------------------------- conv1_2's data gradient with conv1_1's weight gradient
def _check_w1g(n, h, w, dtype, beta, red=None, launch=lambda fn: fn(), seed=110):
    """dX against the exact masked data gradient; dW1 / db1 against the exact first-layer weight gradient of the
    ROUNDED dX (the kernel feeds the 16-bit tile it stores to the MFMA).  db1 sums a channel of dX over every pixel, as a
    bias partial does: the operands are the bias-partial family's (sparse, R.W_BP), the image is {-1, 0, 1}."""
    C, _, _ = _mods()
    dens = R.sparse_density(576, n * h * w)
    shift = R.W_BP[2]
    dy16, dy = R.int_operand((n, h, w, 64), R.X_ACT, dtype, seed, DEV, density=dens)
    w16, wt = R.int_operand((64, 64, 3, 3), R.W_BP, dtype, seed + 1, DEV, density=dens)
    mask16, mask = R.int_operand((n, h, w, 64), MASK_RANGE, dtype, seed + 2, DEV)
    x4 = torch.zeros(n, h, w, 4, dtype=dtype, device=DEV)
    x4[..., :3] = R.int_operand((n, h, w, 3), (-1, 1, 0), dtype, seed + 3, DEV)[0]
    assert R.exactness_bound(lambda a, c: R.dgrad_ref(a, c, 1), (dy, wt), shift) < R.LIMIT
    dx_want = R.to16(R.dgrad_mask_ref(dy, wt, mask), dtype)
    dx64, x464 = dx_want.to(F64), x4.to(F64)
    assert R.exactness_bound(R.wgrad_first_ref, (dx64, x464), shift) + 64 * 2.0 ** shift < R.LIMIT
    gw, gb = R.wgrad_first_ref(dx64, x464)
    cap = C.w1g_slab_cap(DEV)
    if red is not None:
        ncu = cap // 2
        ntile = n * -(-h // 4) * -(-w // 64)
        per = -(-ntile // ncu)
        assert _reduce_kernel(2 * -(-ntile // per), 36, 64, 4, 9, True) == red
    sl = torch.full((cap, 36 * 64), float("nan"), device=DEV)
    bsl = torch.full((cap, 64), float("nan"), device=DEV)
    dw0, dw064 = R.int_operand((64, 3, 3, 3), (-64, 64, 0), torch.float32, seed + 4, DEV)
    db0, db064 = R.int_operand((64,), (-64, 64, 0), torch.float32, seed + 5, DEV)
    dw, db = dw0.clone(), db0.clone()
    dx = launch(lambda: C.conv_dgrad_w1g(dy16, C.pack_weight_dgrad(w16.float(), dtype), mask16, x4, dw, db, slabs=sl,
                                         bslabs=bsl, store_dx=True, beta=beta))
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_want)
    assert torch.equal(dw, R.to32(R.wgrad_update_ref(gw, dw064, beta)))
    assert torch.equal(db, R.to32(R.wgrad_update_ref(gb, db064, beta)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,beta,red", [(2, 40, 128, 0.0, "r4"), (1, 37, 150, 0.0, "r4"), (2, 13, 70, 1.0, "r4"),
                                            (3, 44, 256, 0.5, "r64")])      # 132 tiles: 264 slabs of 36 x 64
def test_dgrad_w1g(n, h, w, beta, red, dtype):
    _check_w1g(n, h, w, dtype, beta, red)


# ------------------------------------------------------------------------------------------------------ degenerate maps
# (n, h, w, dil): one pixel; one row; one column; a row of one 64-pixel stage per image; a map narrower than the dilated
# kernel, where every horizontal side tap falls in the padding; 35 pixels per image, so one pixel tile holds three
# whole images and no tap may reach across an image boundary
DEGENERATE = [(1, 1, 1, 1), (1, 1, 5, 1), (2, 2, 1, 1), (3, 1, 64, 1), (1, 3, 2, 2), (3, 5, 7, 1)]
# family -> (tile, dispatch, Cin values (64 and the family's largest), Cout, epilogues, takes dilation 2)
FAMILIES = {
    "generic": (1, {}, (64, 1024), 128, BASIC, True),
    "v1": (12, {}, (64, 1024), 128, BASIC, True),
    "v2": (22, {"splitk": 0}, (64, 1024), 128, V2, True),
    "v2_auto_splitk": (0, {"splitk": 1, "rring": 0}, (64, 1024), 256, V2, True),
    "halo": (31, {"ws64": 0}, (64,), 128, BASIC, False),
    "ws64": (31, {"ws64": 1}, (64,), 64, BASIC, False),
    "row_ring": (27, {"rring": 2, "splitk": 0}, (64, 1024), 256, ("bias_relu", "mask"), True),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,dil", DEGENERATE)
@pytest.mark.parametrize("family,ci", [(f, ci) for f, v in FAMILIES.items() for ci in v[2]])
def test_degenerate_maps(family, ci, n, h, w, dil, dtype, dispatch_cfg):
    tile, cfg, _, co, epis, dil2 = FAMILIES[family]
    dispatch_cfg(**cfg)
    if dil == 2 and not dil2:
        dil = 1                                            # a dilation-1 kernel: the same 3 x 2 map at dilation 1
    _check_conv(n, h, w, ci, co, 3, dil, tile, dtype, epis, seed=120, launch=_or_skip)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,dil", DEGENERATE)
@pytest.mark.parametrize("tile", [0, 2])
def test_degenerate_maps_first_layer(tile, n, h, w, dil, dtype):
    _check_conv(n, h, w, 4, 64, 3, 1, tile, dtype, ("bias_relu",), seed=121, first=True, launch=_or_skip)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,dil", DEGENERATE)
@pytest.mark.parametrize("ci", [64, 512])
def test_degenerate_maps_batched(ci, n, h, w, dil, dtype):
    C, _, _ = _mods()
    items = [_conv_operands(n, h, w, ci, 128, 3, dtype, 122 + 10 * i) for i in range(2)]
    x = torch.stack([o["x16"] for o in items])
    wp = torch.stack([C.pack_weight_fwd(o["w16"].float(), dtype) for o in items])
    for o in items:
        assert R.exactness_bound(lambda a, c: R.conv_ref(a, c, dil), (o["x"], o["w"]), 6) < R.LIMIT
    got = _or_skip(lambda: C.conv_igemm_batched(x, wp, ksize=3, dil=dil, epi=C.EPI_NONE))
    torch.cuda.synchronize()
    for i, o in enumerate(items):
        assert torch.equal(got[i], R.to16(R.conv_ref(o["x"], o["w"], dil), dtype)), i


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,dil", DEGENERATE)
def test_degenerate_maps_pool_fwd(n, h, w, dil, dtype):
    """The fused pool needs an even H and a W that is a multiple of half its pixel tile: it takes none of these maps."""
    C, _, _ = _mods()
    o = _conv_operands(n, h, w, 64, 128, 3, dtype, 123)
    if C.conv_pool_fwd_ok(o["x16"], 128, 3):
        _check_pool_fwd(n, h, w, 64, 128, dil, 0, dtype, seed=123)
    else:
        wf = C.pack_weight_fwd(o["w16"].float(), dtype)
        _or_skip(lambda: C.conv_pool_fwd(o["x16"], wf, o["b32"], ksize=3, dil=dil, codes=True))
        raise AssertionError("conv_pool_fwd_ok said no and the launch went through")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,dil", DEGENERATE)
def test_degenerate_maps_w1g(n, h, w, dil, dtype):
    _check_w1g(n, h, w, dtype, 0.0, launch=_or_skip, seed=124)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w,dil", DEGENERATE)
@pytest.mark.parametrize("ci,co", [(64, 64), (1024, 512)])
def test_degenerate_maps_wgrad(ci, co, n, h, w, dil, dtype, dispatch_cfg):
    """The generic weight gradient (tap ring off): cfg 3 at 64 -> 64, cfg 9's tiles at 1024 -> 512."""
    C, ext, _ = _mods()
    dispatch_cfg(wgrad_tap=0)
    _check_wgrad(n, h, w, ci, co, 3, dil, dtype, 3 if ci == 64 else 9, launch=_or_skip, seed=125)
