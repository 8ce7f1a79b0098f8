"""The context module's fp32 cell GEMMs (csrc/context.hip can_ctx_gemm: ctx_mm_kernel on the fp32 matrix cores,
ctx_gemm_kernel on 32 x 64 LDS tiles) and ctx_w2_scatter_kernel, bit for bit.

Operands are exactly representable, as in tests/conv_exact_reference.py: the cell tables are small integers, the
weights integers times 2^-6, all fp32.  Every product and every partial sum, in any order, is then a multiple of one
unit, and while the sum of the absolute values of an output's terms (the ``beta * old`` term included) stays below
2^24 units -- asserted with ``exactness_bound`` -- every partial sum is exact in fp32.  The matrix-core kernel (K split
over 8 waves, permuted K order), the tiled kernel and the fp64 reference (tests/ctx_reference.py, rounded by ``to32``)
must therefore agree bit for bit: every comparison is ``torch.equal`` and there is no tolerance.

Which of the two kernels a case runs is asserted through ``ctx_gemm_form``, the rule the launcher itself decides by.
"""
import pytest
import torch

import conv_exact_reference as X
import ctx_reference as R
from ctx_reference import CELL_OFF, SCALES

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
CELLS = X.X_ACT                      # cell tables (ave, u, dA, dt): integers in [-12, 12]
WEIGHTS = X.W_FWD                    # conv{S}_1 / conv{S}_2 weights: integers in [-32, 32] times 2^-6
OLD = (-64, 64, 0)                   # what the output holds before an accumulating launch
BETAS = (0.0, 1.0, 0.5)

# (N, C, form): 1 the matrix-core kernel, 0 the tiled one.  (14, 64): the largest batch of the matrix-core form, scale
# 6 has 504 rows (the last 16-chunk of K half full in mode 2) and scale 1 has 14 (fewer than one 16-row tile);
# (15, 64): the smallest batch of the tiled form; (2, 576): C > 512, the tiled form with partial 32-row tiles.
CASES = [(1, 64, 1), (3, 128, 1), (14, 64, 1), (8, 512, 1), (15, 64, 0), (15, 512, 0), (2, 576, 0)]
_forms_run = set()
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _both_forms_ran():
    yield
    print(f"\nCTX-GEMM forms run (ctx_gemm_form): {sorted(_forms_run)}")


def _ext():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _case(n, c):
    """Operands and fp64 references of a case, made once and left unchanged: x, d cell tables [N, 50, C], W [4, C, C]
    and the three products."""
    got = _cache.get((n, c))
    if got is None:
        x32, x = X.int_operand((n, 50, c), CELLS, torch.float32, 7 * n + c, DEV)
        d32, d = X.int_operand((n, 50, c), CELLS, torch.float32, 7 * n + c + 1, DEV)
        w32, w = X.int_operand((4, c, c), WEIGHTS, torch.float32, 7 * n + c + 2, DEV)
        got = _cache[(n, c)] = dict(x32=x32, x=x, d32=d32, d=d, w32=w32, w=w, fwd=R.conv1x1_cells(x, w),
                                    bwd=R.conv1x1_cells_t(d, w), dw=R.wgrad_cells(d, x))
    return got


def _check_form(ext, n, c, form):
    assert ext.ctx_gemm_form(n, c) == form, (n, c, ext.ctx_gemm_form(n, c))
    _forms_run.add(form)


def _prefill(shape, beta, seed):
    """(the output buffer before the launch, its fp64 value or None): NaN at beta = 0 (the old value must not be
    read), small integers otherwise."""
    if beta == 0.0:
        return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV), None
    return X.int_operand(shape, OLD, torch.float32, seed, DEV)


def _launch_cells(ext, mode, src, w32, out, n, c, beta):
    # scale = 1 and no dscale: both kernels ignore them in modes 0 and 1 (ctx_mm_kernel's sc is 1 there, the tiled
    # kernel's epilogue does not multiply), which is what the callers in ops/context_exec.py rely on
    ext.ctx_gemm(mode, src.data_ptr(), 0, [w32[i].data_ptr() for i in range(4)], out.data_ptr(), [], n, c, beta, 1.0,
                 0, _stream())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,c,form", CASES)
def test_cell_gemm_forward_and_data_gradient(n, c, form, mode):
    """Mode 0, table = cells W^T, and mode 1, dave = dA W (``beta = 1``: du += W2^T dt): all 50 cell rows of every
    image, at beta 0 / 1 / 0.5."""
    ext = _ext()
    _check_form(ext, n, c, form)
    k = _case(n, c)
    src32, src, ref = (k["x32"], k["x"], k["fwd"]) if mode == 0 else (k["d32"], k["d"], k["bwd"])
    fn = R.conv1x1_cells if mode == 0 else R.conv1x1_cells_t
    shift = WEIGHTS[2]
    # units of 2^-6; the old value, |old| <= 64, adds at most 64 * 2^6 units (beta <= 1, and beta = 0.5 of an integer
    # is a whole number of units)
    assert X.exactness_bound(fn, (src, k["w"]), shift) + 64 * 2.0 ** shift < X.LIMIT
    for beta in BETAS:
        out, old = _prefill((n, 50, c), beta, 1000 + mode)
        _launch_cells(ext, mode, src32, k["w32"], out, n, c, beta)
        torch.cuda.synchronize()
        want = X.to32(ref if old is None else beta * old + ref)
        assert torch.equal(out, want), f"beta {beta}: {int((out != want).sum())} of {want.numel()} elements differ"


@pytest.mark.parametrize("n,c,form", CASES)
def test_cell_gemm_weight_gradient(n, c, form):
    """Mode 2, gw_S = beta gw0_S + scale dscale dA_S^T ave_S with scale = 0.25 and dscale absent or a device scalar
    2^-3: every element of the four [C][C] buffers."""
    ext = _ext()
    _check_form(ext, n, c, form)
    k = _case(n, c)
    scale = 0.25
    for dscale_k in (None, 3):
        ds = 1.0 if dscale_k is None else 2.0 ** -dscale_k
        dsc = None if dscale_k is None else torch.tensor([ds], dtype=torch.float32, device=DEV)
        # in units of scale * dscale (a power of two): the product's bound plus the beta * gw0 term
        assert X.exactness_bound(R.wgrad_cells, (k["d"], k["x"]), 0) + 64 / (scale * ds) < X.LIMIT
        for beta in BETAS:
            gw, old = _prefill((4, c, c), beta, 2000)
            ext.ctx_gemm(2, k["d32"].data_ptr(), k["x32"].data_ptr(), [], 0, [gw[i].data_ptr() for i in range(4)], n,
                         c, beta, scale, 0 if dsc is None else dsc.data_ptr(), _stream())
            torch.cuda.synchronize()
            fresh = (scale * ds) * k["dw"]
            want = X.to32(fresh if old is None else beta * old + fresh)
            for si, S in enumerate(SCALES):
                assert torch.equal(gw[si], want[si]), \
                    f"scale {S}, beta {beta}, dscale {dscale_k}: {int((gw[si] != want[si]).sum())} elements differ"


@pytest.mark.parametrize("mode", [0, 1])
def test_cell_gemm_batch_isolation(mode):
    """(3, 128) twice, image 1 changed in between: the rows of images 0 and 2 come out bitwise unchanged."""
    ext = _ext()
    n, c = 3, 128
    _check_form(ext, n, c, 1)
    k = _case(n, c)
    src = (k["x32"] if mode == 0 else k["d32"]).clone()
    a = torch.full((n, 50, c), float("nan"), dtype=torch.float32, device=DEV)
    _launch_cells(ext, mode, src, k["w32"], a, n, c, 0.0)
    src[1] = X.int_operand((50, c), CELLS, torch.float32, 99, DEV)[0]
    b = torch.full_like(a, float("nan"))
    _launch_cells(ext, mode, src, k["w32"], b, n, c, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert not torch.equal(a[1], b[1])
    assert torch.equal(a, X.to32(k["fwd"] if mode == 0 else k["bwd"]))


def test_refused_shapes():
    """What ctx_gemm_form refuses, ctx_gemm refuses with the same code before any launch."""
    ext = _ext()
    t = torch.zeros(50 * 96, device=DEV)
    for n, c in ((1, 96), (0, 64), (1, 0)):
        assert ext.ctx_gemm_form(n, c) == -2
        with pytest.raises(RuntimeError, match="rc=-2"):
            ext.ctx_gemm(0, t.data_ptr(), 0, [t.data_ptr()] * 4, t.data_ptr(), [], n, c, 0.0, 1.0, 0, _stream())


# --------------------------------------------------------------------------------------------------------- the scatter
@pytest.mark.parametrize("c", [64, 512, 1024])
def test_w2_scatter(c):
    """ctx_w2_scatter_kernel: d_S[c] = beta d_S[c] + tmp[4c + si], the interleaved rows of the linearised dW2cat back
    into the four conv{S}_2 gradients.  Integer tmp and old values: exact.  C = 1024 is the smallest size at which the
    grid cap of 2048 blocks makes the grid-stride loop take a second pass (C^2 float4 items over 256 threads)."""
    ext = _ext()
    assert (c * c + 255) // 256 > 2048 if c == 1024 else (c * c + 255) // 256 <= 2048
    tmp32, tmp = X.int_operand((4 * c, c), (-1000, 1000, 0), torch.float32, 31 + c, DEV)
    rows = tmp.view(c, 4, c)                                     # [c][si][k]: row 4c + si
    for beta in BETAS:
        d, old = _prefill((4, c, c), beta, 3000 + c)
        ext.ctx_w2_scatter(tmp32.data_ptr(), [d[i].data_ptr() for i in range(4)], c, beta, _stream())
        torch.cuda.synchronize()
        for si, S in enumerate(SCALES):
            want = X.to32(rows[:, si] if old is None else beta * old[si] + rows[:, si])
            assert torch.equal(d[si], want), f"scale {S}, beta {beta}: {int((d[si] != want).sum())} elements differ"


def test_cases_cover_both_forms():
    ext = _ext()
    assert {ext.ctx_gemm_form(n, c) for n, c, _ in CASES} == {0, 1}
    assert tuple(CELL_OFF) == (0, 1, 5, 14) and sum(S * S for S in SCALES) == 50      # the [N, 50, C] layout used here
