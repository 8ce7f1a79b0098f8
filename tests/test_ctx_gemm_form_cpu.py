"""The kernel choice of the context module's cell GEMMs (csrc/context.hip can_ctx_gemm_form, binding ctx_gemm_form)
without a GPU: 1 the matrix-core kernel (K <= 512 on both sides: C channels and the N * 36 cell rows of scale 6), 0
the tiled kernel, -2 what can_ctx_gemm refuses.  Host code only; can_ctx_gemm decides by the same function."""
import pytest


@pytest.fixture(scope="module")
def ext():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require()


def test_form_rule(ext):
    for c in range(64, 1025, 64):
        for n in range(1, 40):
            assert ext.ctx_gemm_form(n, c) == int(c <= 512 and n * 36 <= 512), (n, c)
    # the boundary in the batch: 14 * 36 = 504 <= 512 < 540 = 15 * 36; and in the channels
    assert [ext.ctx_gemm_form(n, 512) for n in (14, 15)] == [1, 0]
    assert [ext.ctx_gemm_form(2, c) for c in (512, 576)] == [1, 0]


@pytest.mark.parametrize("n,c", [(0, 64), (-1, 512), (1, 0), (1, 32), (1, 96), (8, 520), (1, -64)])
def test_refused(ext, n, c):
    assert ext.ctx_gemm_form(n, c) == -2
