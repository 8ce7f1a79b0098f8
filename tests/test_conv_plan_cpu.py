"""The conv launch planner (csrc/conv_plan.h plan_conv, binding conv_launch_plan) without a GPU.

tests/golden/conv_plan_parent.json holds what conv_plan / splitk_plan / conv_pool_tp answered, on a 256-CU MI355X, at
the commit before the planner existed (scripts/dev/dump_conv_plans.py: every conv of the network at four input sizes
and every conv shape of the GPU conv tests, epilogues 0-7, 96 dispatch variants).  Those three functions re-implemented
the launcher's choice by hand; plan_conv is the choice the launchers execute, and it must reproduce every recorded
answer, with these exceptions, each an input where the old query answered for a launch the launcher does not make:

* EPI_POOLFWD (6).  The old conv_plan answered with conv_igemm's choice for the shape (halo kernel for 64 -> 64 / 128,
  else the LDS-DMA default tile); conv_igemm does not take that epilogue.  The plan is conv_pool_fwd's launch:
  27 (row ring) for a 3x3 dilation-1 Cout % 256 layer with H even and W % 128 == 0 under dispatch rring_pool,
  33 / 31 (dispatch ws64) for 64 -> 64 with H % 4 == 0 and W % 64 == 0 (-13 otherwise), else the LDS-DMA default tile
  (what the old query answered for EPI_SIGMOID, which no other kernel family takes) when H is even and W a multiple of
  half its pixel tile, else -12.  Split-K: 1 for the halo kernels; the row-ring pool tiles are the LDS-DMA tiles of the
  same map (256 x 256), so both match the recorded EPI_SIGMOID factor.
* H < 2 or W < 2: the LDS-DMA / row-ring launchers return -7 (conv_pool_fwd -3, and -19 for an odd width, whose
  last pool window would straddle the valid columns); the old queries had no shape guards.
* conv_pool_tp with an explicit tile whose channel count does not divide Cout: the launch returns -8, the answer is 0.
"""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI_MASK, EPI_SIGMOID, EPI_POOLBWD, EPI_POOLFWD = 1, 4, 5, 6
V2_POOL_TP = {21: 256, 22: 256, 23: 512, 25: 512}


@pytest.fixture(scope="module")
def fix():
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ext():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require()


def _variants(fix):
    from can_distributed_pytorch_amd.ops import dispatch
    for i, var in enumerate(fix["variants"]):
        kw = dict(zip(fix["keys"], var))
        with dispatch.override(**kw):
            yield i, kw


def _pool_expected(kw, h, w, ci, co, k, dil, lds):
    """conv_pool_fwd's launch (module docstring); lds = the LDS-DMA default tile of the layer."""
    if h < 2 or w < 2:
        return -3
    if w % 2:
        return -19          # the valid width (here the whole row) must hold whole pool windows
    if k == 3 and dil == 1 and h % 2 == 0 and w % 128 == 0 and kw["rring_pool"] and co % 256 == 0:
        return 27
    if ci == 64 and co == 64 and k == 3 and dil == 1:
        return -13 if (h % 4 or w % 64) else (33 if kw["ws64"] else 31)
    return lds if (h % 2 == 0 and w % (V2_POOL_TP[lds] // 2) == 0) else -12


def test_plans_reproduce_the_parent(fix, ext):
    ncu, vecs, table = fix["ncu"], fix["vecs"], ext.conv_tile_table()
    assert ncu > 0
    checked = 0
    for i, kw in _variants(fix):
        for n, h, w, ci, co, k, dil, plan_ids, sk_ids in fix["rows"]:
            for epi in range(8):
                pool = epi == EPI_POOLFWD
                p = ext.conv_launch_plan(n, h, w, ci, co, k, dil, epi, entry=int(pool), ncu=ncu)
                got = p["err"] or p["cfg"]
                where = (kw, n, h, w, ci, co, k, dil, epi, p)
                want_cfg, want_ks = vecs[plan_ids[epi]][i], vecs[sk_ids[epi]][i]
                if pool:
                    want_cfg = _pool_expected(kw, h, w, ci, co, k, dil, vecs[plan_ids[EPI_SIGMOID]][i])
                    want_ks = 1 if want_cfg in (31, 33) else vecs[sk_ids[EPI_SIGMOID]][i]
                elif h < 2 or w < 2:
                    want_cfg = want_cfg if want_cfg in (31, 33) else -7      # the halo kernels take one-row maps
                assert got == want_cfg, where
                if p["err"]:
                    continue
                assert p["ks"] == want_ks, where
                assert p["cfg"] in table, where
                # naming the planned config gives the same launch (33 is not a tile= value: the ws64 form of 31,
                # chosen by dispatch ws64; the pool entry's halo kernel is its tile 0 only)
                if not (pool and p["cfg"] in (31, 33)):
                    tile = 31 if p["cfg"] == 33 else p["cfg"]
                    assert ext.conv_launch_plan(n, h, w, ci, co, k, dil, epi, tile_cfg=tile, entry=int(pool),
                                                ncu=ncu) == p, where
                checked += 1
    assert checked > 100000


def test_pool_tp_reproduces_the_parent(fix, ext):
    table = ext.conv_tile_table()
    for i, kw in _variants(fix):
        for ci, co, k, tile, vid in fix["pool_tp"]:
            want = fix["vecs"][vid][i]
            if tile and tile in table and table[tile]["TC"] and co % table[tile]["TC"]:
                want = 0
            assert ext.conv_pool_tp(ci, co, k, tile) == want, (kw, ci, co, k, tile)


def test_bias_partial_capacity_covers_every_plan(fix, ext):
    """The table-derived capacity holds the rows of every plan, and is never larger than the hand-written bound it
    replaces (LDS-DMA ceil(M / 64) + 64, halo 8 per 4 x 64 tile, row ring 4 per 2 x 128 / 8 per 4 x 128 tile)."""
    from can_distributed_pytorch_amd.ops import conv as C
    ncu = fix["ncu"]
    for i, kw in _variants(fix):
        for n, h, w, ci, co, k, dil, _, _ in fix["rows"]:
            cap = C.bias_part_capacity(n, h, w)
            cb = -(-w // 128)
            assert cap <= max(-(-n * h * w // 64) + 64, n * (-(-h // 4)) * (-(-w // 64)) * 8,
                              n * (-(-h // 2)) * cb * 4, n * (-(-h // 4)) * cb * 8)
            for epi in (EPI_MASK, EPI_POOLBWD):
                for tile in (0, 11, 12, 13, 21, 22, 23, 25, 27, 28, 29, 31):
                    p = ext.conv_launch_plan(n, h, w, ci, co, k, dil, epi, tile_cfg=tile, want_bpart=True,
                                             bpart_cap=1 << 30, ncu=ncu)
                    assert p["err"] or 0 <= p["bpart_rows"] <= cap, (kw, n, h, w, ci, co, k, dil, epi, tile, p)
                    small = ext.conv_launch_plan(n, h, w, ci, co, k, dil, epi, tile_cfg=tile, want_bpart=True,
                                                 bpart_cap=cap, ncu=ncu)
                    assert small["err"] or small["bpart_rows"] == p["bpart_rows"]
        if i >= 7:
            break       # the rows depend on rring / rring128 / ws64 only through the config: 8 variants name them all


def test_sign_bit_and_error_rules(ext):
    """What the shape-only queries cannot say: sign-bit masks move a 64 -> 64 / 128 data gradient off the halo kernel,
    and the launcher's refusals keep their codes."""
    from can_distributed_pytorch_amd.ops import conv as C, dispatch
    plan = lambda *a, **kw: ext.conv_launch_plan(*a, ncu=256, **kw)
    with dispatch.override(rring=0):
        assert plan(1, 64, 256, 64, 128, 3, 1, EPI_MASK)["cfg"] == 31
        assert plan(1, 64, 256, 64, 128, 3, 1, EPI_MASK, mbits_in=True)["cfg"] == 25
    assert plan(1, 64, 256, 64, 64, 3, 1, EPI_MASK, mbits_in=True)["err"] == -17       # row ring 28 takes no bits
    assert plan(1, 64, 256, 64, 128, 3, 1, 0, mbits_out=True)["cfg"] == 31
    assert plan(1, 64, 256, 64, 64, 3, 1, 0, mbits_out=True)["err"] == -18
    assert plan(1, 64, 256, 4, 64, 3, 1, 0, first=1, mbits_out=True)["cfg"] == 32
    assert plan(1, 64, 256, 96, 64, 3, 1, 0)["err"] == -3 and plan(1, 64, 256, 64, 96, 3, 1, 0)["err"] == -2
    assert plan(1, 64, 256, 128, 128, 3, 1, 0, tile_cfg=21)["err"] == -8
    assert plan(1, 64, 256, 128, 128, 3, 1, 0, tile_cfg=33)["err"] == -9
    assert plan(1, 64, 250, 128, 128, 3, 1, 0, tile_cfg=27)["err"] == -16
    assert plan(1, 64, 256, 128, 128, 3, 1, 0, tile_cfg=2, wv=200)["err"] == -19
    assert plan(1, 64, 256, 128, 128, 3, 1, 0, entry=2, nb=4, tile_cfg=27)["err"] == -8
    # a bias-partial buffer that fits keeps 64 -> 64 on the halo kernel (ws64 writes none)
    p = plan(2, 16, 96, 64, 64, 3, 1, EPI_MASK, want_bpart=True, bpart_cap=C.bias_part_capacity(2, 16, 96))
    assert p["cfg"] == 31 and p["bpart_rows"] == 2 * 4 * 2 * 4
    assert plan(2, 16, 96, 64, 64, 3, 1, EPI_MASK, want_bpart=True, bpart_cap=8)["cfg"] == 33
    # the front end's questions
    assert C.mask_bits_out_ok(64, 128) and C.mask_bits_out_ok(3, 64, first=True)
    assert not C.mask_bits_out_ok(64, 64) and not C.mask_bits_out_ok(64, 128, dil=2)
    assert C.mask_bits_ok(384, 512, 128, 128) and not C.mask_bits_ok(384, 512, 128, 64)
