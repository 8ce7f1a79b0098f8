"""On the device: the query names the tests use (conv_plan, splitk_plan) are views of the plan the launchers execute
(csrc/conv_plan.h; the planner itself is checked without a GPU in tests/test_conv_plan_cpu.py), and a launch writes the
bias-partial rows its plan names."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPI_BIAS_RELU, EPI_MASK, EPI_POOLBWD, EPI_F32 = 0, 1, 5, 7
SHAPES = [(1, 6, 256, 256, 256, 1), (1, 48, 128, 512, 128, 1), (1, 30, 40, 512, 256, 2), (2, 8, 128, 64, 64, 1)]


def _mods():
    from can_distributed_pytorch_amd.ops import _ext
    from can_distributed_pytorch_amd.ops import conv as C
    return C, _ext.require()


@pytest.mark.parametrize("n,h,w,ci,co,dil", SHAPES)
def test_query_names_are_views_of_the_plan(n, h, w, ci, co, dil):
    _, ext = _mods()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for epi in (EPI_BIAS_RELU, EPI_MASK, EPI_POOLBWD, EPI_F32):
        p = ext.conv_launch_plan(n, h, w, ci, co, 3, dil, epi, ncu=ncu)
        assert p["err"] == 0 and p == ext.conv_launch_plan(n, h, w, ci, co, 3, dil, epi)     # ncu 0: the device's
        assert ext.conv_plan(h, w, ci, co, 3, dil, epi) == p["cfg"]
        assert ext.splitk_plan(n, h, w, ci, co, 3, dil, epi) == p["ks"]


def test_launch_writes_the_planned_bias_partial_rows():
    C, ext = _mods()
    n, h, w, c = 2, 6, 256, 256
    g = torch.Generator(device="cuda").manual_seed(0)
    dy = torch.randn(n, h, w, c, device="cuda", generator=g).to(torch.bfloat16)
    mask = torch.randn(n, h, w, c, device="cuda", generator=g).to(torch.bfloat16)
    pack = C.pack_weight_dgrad(torch.randn(c, c, 3, 3, device="cuda", generator=g) * 0.05)
    cap = C.bias_part_capacity(n, h, w)
    bp = torch.full((cap, c), float("nan"), device="cuda")
    dx, part = C.conv_igemm(dy, pack, None, ksize=3, epi=EPI_MASK, mask=mask, bias_part=bp)
    torch.cuda.synchronize()
    p = ext.conv_launch_plan(n, h, w, c, c, 3, 1, EPI_MASK, want_bpart=True, bpart_cap=cap)
    assert p["err"] == 0 and p["bpart_rows"] > 0
    assert part is not None and part.shape[0] == p["bpart_rows"]
    assert tuple(dx.shape) == (n, h, w, c)
    assert torch.isfinite(bp[:p["bpart_rows"]]).all() and torch.isnan(bp[p["bpart_rows"]:]).all()
