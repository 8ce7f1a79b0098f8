"""The weight-gradient launch planner (csrc/wgrad_plan.h plan_wgrad, binding wgrad_launch_plan) without a GPU.

tests/golden/wgrad_plan_parent.json holds what wgrad_plan / WgradWorkspace.plan / wgrad_1x1_batched_plan answered for
256 CUs at the commit before the planner existed (scripts/dev/dump_wgrad_plans.py: every conv of the network at four
input sizes, every conv shape of the GPU conv tests in both channel orders and the first layer; dispatch wgrad_tap 0-3;
the map width given and unknown).  plan_wgrad is the choice the launcher executes, and it must reproduce every recorded
S, mslice, cfg and workspace size, through the dict binding, the old tuple binding and WgradWorkspace.plan.  The two
old queries know M and W only and keep every answer; the dict binding, given the image height as the launcher is,
answers a map under 2 x 2 off the tap ring with the launcher's -3 (and with the recorded values when the height is
withheld).

What the old launcher decided at launch time could not be recorded; ``_launch_expected`` restates it from
conv_wgrad.hip at that commit (75a34c0):

* family of cfg 9 / 10 / 11 (lines 1365-1397): v2 when ``(W % 64 == 0 or rw)``, ``Cin % tk == 0``, ``K % tk == 0``
  (tk = 256 / 128 / 256), the v2 slice length is a multiple of 64, ``M * Cout * 2 < 2^31 - 1`` and ``Cout <= 2048``;
  else the v1 kernel of cfg 7 / 2 / 6.  ``rw`` (line 1311): a 3x3 layer on a width that is no multiple of 64; then
  (lines 1313-1316) the launch counts virtual pixels, ``vM = N H ceil(W / 64) 64`` in slices of
  ``ceil(ceil(vM / S) / 64) 64``.
* bias mode: no db, no bias work (line 1270); external partials (lines 1268, 1280-1288) are read in place up to 512
  rows, longer lists are folded to ``ceil(rows / ceil(rows / 512))`` rows; else the v2 and tap-ring kernels are
  preceded by the 512-row column sum (lines 1319-1322, 1369-1372, 1385-1388) and every other kernel writes S rows.
* slab reduction (launch_reduce2, lines 1090-1107): as ``_reduce_kernel`` of tests/test_gpu_conv_exact.py.
"""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WG_FIRST, WG_GLDS, WG_GLDS2, WG_TAP, WG_HALO = range(5)          # WgradFamily of wgrad_plan.h
WB_NONE, WB_KERNEL, WB_COLSUM, WB_EXT, WB_EXT_FOLD = range(5)    # WgradBias
RED_TILED, RED_1, RED_4, RED_16, RED_64 = 0, 1, 4, 16, 64        # WgradReduce
V2_TK = {9: 256, 10: 128, 11: 256}
V2_FALLBACK = {9: 7, 10: 2, 11: 6}


@pytest.fixture(scope="module")
def fix():
    with open(os.path.join(ROOT, "tests", "golden", "wgrad_plan_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ext():
    from can_distributed_pytorch_amd.ops import _ext
    return _ext.require()


def _device_cus():
    """What the bindings without an ncu argument plan for: the device's CUs, 256 without one."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _ceil(a, b):
    return -(-a // b)


def _launch_expected(n, h, w, ci, co, k, dil, first, s, mslice, cfg, want_db, bext_rows):
    """family, ragged, vM, vmslice, bias mode, Sb, Sb_ext, bias_rpb, reduce of the old launcher (module docstring)."""
    M, K = n * h * w, 64 if first else k * k * ci
    fam = {0: WG_FIRST, 8: WG_HALO, 12: WG_TAP}.get(cfg, WG_GLDS)
    ragged, vM, vms = False, 0, 0
    if cfg in V2_TK:
        rw = w % 64 != 0 and k == 3
        gM = n * h * _ceil(w, 64) * 64 if rw else M
        gms = _ceil(_ceil(gM, s), 64) * 64 if rw else mslice
        if (w % 64 == 0 or rw) and ci % V2_TK[cfg] == 0 and K % V2_TK[cfg] == 0 and gms % 64 == 0 and \
                M * co * 2 < 0x7fffffff and co <= 2048:
            fam, ragged, vM, vms = WG_GLDS2, rw, gM, gms
    bias, sb, sb_ext, rpb = WB_NONE, s, 0, 0
    if want_db and bext_rows > 0:
        if bext_rows <= 512:
            bias, sb_ext = WB_EXT, bext_rows
        else:
            rpb = _ceil(bext_rows, 512)
            bias, sb_ext = WB_EXT_FOLD, _ceil(bext_rows, rpb)
    elif want_db:
        bias = WB_COLSUM if fam in (WG_GLDS2, WG_TAP) else WB_KERNEL
        sb = 512 if bias == WB_COLSUM else s
    cin_r, taps = (4, 9) if first else (ci, k * k)
    if not first and taps == 9 and s <= 16 and co % 64 == 0 and cin_r % 8 == 0 and (co // 64) * (cin_r // 8) >= 256:
        red = RED_TILED
    elif s <= 16:
        red = RED_1
    elif s <= 128:
        red = RED_4
    else:
        red = RED_64 if K * co < 4096 else RED_16
    return dict(family=fam, ragged=ragged, vM=vM, vmslice=vms, bias=bias, Sb=sb, Sb_ext=sb_ext, bias_rpb=rpb,
                reduce=red)


def _check_invariants(p, table, n, h, w, ci, co, k, first, where):
    M, K = n * h * w, 64 if first else k * k * ci
    assert p["cfg"] in table and p["S"] >= 1 and p["blocks"] == p["ntile"] * p["S"] > 0, where
    t = table[p["cfg"]]
    if p["family"] in (WG_FIRST, WG_GLDS, WG_GLDS2):
        assert p["S"] * p["mslice"] >= M and p["mslice"] % t["BKM"] == 0, where
        assert p["ntile"] == (co // t["TCo"]) * _ceil(K, t["TK"]), where
        if p["family"] == WG_GLDS2:
            assert p["S"] * p["vmslice"] >= p["vM"] >= M and p["vmslice"] % t["BKM"] == 0, where
        elif p["cfg"] in V2_FALLBACK:
            v1 = table[t["v1"]]
            assert t["v1"] == V2_FALLBACK[p["cfg"]] and (v1["TCo"], v1["TK"], v1["BKM"]) == (t["TCo"], t["TK"], t["BKM"])
    if p["family"] == WG_TAP:
        assert p["S"] <= p["tap_total"] <= p["S"] * p["tap_spb"], where
    if p["family"] == WG_HALO and w:
        assert p["halo_tiles"] <= p["S"] * p["halo_tps"], where
    assert p["Sb_ext"] <= 512, where
    rows = {WB_NONE: 0, WB_KERNEL: p["S"], WB_COLSUM: p["Sb"], WB_EXT: 0, WB_EXT_FOLD: p["Sb_ext"]}[p["bias"]]
    assert p["bias_off"] == p["S"] * K * co and p["bias_off"] + rows * co <= p["ws_floats"], where


def test_plans_reproduce_the_parent(fix, ext):
    from can_distributed_pytorch_amd.ops import conv as C, dispatch
    ncu, vecs, table = fix["ncu"], fix["vecs"], ext.wgrad_tile_table()
    assert ncu > 0 and 5 not in table
    old_too = _device_cus() == ncu        # the bindings without an ncu argument plan for the device they find
    ws = C.WgradWorkspace("cpu")
    checked, cfgs = 0, set()
    for ti, tap in enumerate(fix["taps"]):
        with dispatch.override(wgrad_tap=tap):
            for n, h, w, ci, co, k, dil, first, vid in fix["rows"]:
                M = n * h * w
                for j, wq in enumerate((w, 0)):
                    want = vecs[vid][2 * ti + j]
                    where = (tap, n, h, w, ci, co, k, dil, first, wq, want)
                    if old_too:
                        assert list(ext.wgrad_plan(M, ci, co, k, first, 1024, dil, wq)) == want[:3], where
                        assert list(ws.plan(M, ci, co, k, bool(first), dil, wq)) == want, where
                    p = ext.wgrad_launch_plan(n, h if wq else 0, wq, M, ci, co, k, dil, first, want_db=True, ncu=ncu)
                    if wq and (h < 2 or w < 2) and want[2] != 12:
                        assert p["err"] == -3, where
                        p = ext.wgrad_launch_plan(n, 0, wq, M, ci, co, k, dil, first, want_db=True, ncu=ncu)
                        assert [p["err"], p["S"], p["mslice"], p["cfg"], p["ws_floats"]] == [0] + want, (where, p)
                        continue
                    assert [p["err"], p["S"], p["mslice"], p["cfg"], p["ws_floats"]] == [0] + want, (where, p)
                    _check_invariants(p, table, n, h, wq, ci, co, k, first, where)
                    checked += 1
                    cfgs.add(p["cfg"])
                    if not wq:
                        continue
                    # what the launcher used to decide for itself, in each bias mode
                    for want_db, rows in ((True, 0), (False, 0), (False, 300), (True, 300), (True, 5000)):
                        if rows and want_db and co > 1024:
                            continue
                        q = ext.wgrad_launch_plan(n, h, w, M, ci, co, k, dil, first, want_db=want_db, bext_rows=rows,
                                                  ncu=ncu)
                        exp = _launch_expected(n, h, w, ci, co, k, dil, first, want[0], want[1], want[2], want_db, rows)
                        assert {key: q[key] for key in exp} == exp, (where, want_db, rows, q)
                        assert [q["S"], q["mslice"], q["cfg"], q["ws_floats"]] == want, where
                        _check_invariants(q, table, n, h, w, ci, co, k, first, where)
    assert checked > 2000
    assert cfgs == set(range(13)) - {5}


def test_batched_plans_reproduce_the_parent(fix, ext):
    from can_distributed_pytorch_amd.ops import conv as C
    for m, nb, ci, co, ncu, s, mslice, need in fix["batched"]:
        assert list(C.wgrad_1x1_batched_plan(m, nb, ci, co, ncu=ncu)) == [s, mslice, need]
        p = ext.wgrad_1x1_batched_launch_plan(m, 64, ci, co, nb, ncu)
        assert [p["S"], p["mslice"], p["ws_floats"]] == [s, mslice, need] and p["err"] == (-3 if m % 64 else 0)
        assert p["S"] * p["mslice"] >= m and p["mslice"] % 64 == 0 and need == nb * s * ci * co


def test_tile_table(ext):
    table = ext.wgrad_tile_table()
    assert sorted(table) == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12]
    fams = {c: table[c]["family"] for c in table}
    assert fams == {0: WG_FIRST, 1: WG_GLDS, 2: WG_GLDS, 3: WG_GLDS, 4: WG_GLDS, 6: WG_GLDS, 7: WG_GLDS, 8: WG_HALO,
                    9: WG_GLDS2, 10: WG_GLDS2, 11: WG_GLDS2, 12: WG_TAP}
    assert {c: table[c]["v1"] for c in V2_FALLBACK} == V2_FALLBACK
    assert ext.WGRAD_BIAS_PARTS == 512


def test_error_codes(ext):
    """The launcher's refusals keep their codes, and come from the plan."""
    plan = lambda n, h, w, ci, co, k, **kw: ext.wgrad_launch_plan(n, h, w, n * h * w, ci, co, k, ncu=256, **kw)
    assert plan(1, 16, 64, 3, 64, 3, first=1)["err"] == -2
    assert plan(1, 16, 64, 4, 96, 3, first=1)["err"] == -2
    assert plan(1, 16, 64, 4, 64, 3, first=1)["err"] == 0
    assert plan(1, 16, 64, 96, 128, 3)["err"] == -3 and plan(1, 16, 64, 128, 96, 3)["err"] == -3
    assert plan(1, 16, 64, 0, 128, 3)["err"] == -3 and plan(1, 0, 64, 64, 128, 3)["err"] == -3
    from can_distributed_pytorch_amd.ops import dispatch
    with dispatch.override(wgrad_tap=1):
        assert plan(1, 1, 64, 64, 128, 1)["err"] == -3        # one row, 1x1: off the tap ring
        assert plan(1, 1, 64, 64, 128, 3)["cfg"] == 12        # the tap ring takes one-row maps
    with dispatch.override(wgrad_tap=0):
        assert plan(1, 1, 64, 64, 128, 3)["err"] == -3
    assert plan(1, 16, 64, 9 * 4096, 8192, 3)["err"] == -9    # K * Cout >= 2^31 - 1
    assert plan(1, 16, 64, 512, 2048, 3, want_db=True, bext_rows=8)["err"] == -15
    assert plan(1, 16, 64, 512, 2048, 3, want_db=False, bext_rows=8)["err"] == 0
    assert plan(1, 16, 64, 512, 1024, 3, want_db=True, bext_rows=8)["bias"] == WB_EXT
    bp = lambda m, w, ci, co, nb=4, ncu=224: ext.wgrad_1x1_batched_launch_plan(m, w, ci, co, nb, ncu)["err"]
    assert bp(3072, 128, 512, 512) == 0 and bp(3072, 0, 512, 512) == 0
    assert bp(3072, 128, 512, 384) == -3 and bp(3072, 128, 384, 512) == -3      # channels % 256
    assert bp(3072, 96, 512, 512) == -3                                         # W % 64
    assert bp(3040, 128, 512, 512) == -3                                        # M % 64
    assert bp(2 ** 21, 128, 512, 512) == -3 and bp(2 ** 21 - 64, 128, 512, 512) == 0   # 32-bit operand addressing
    assert bp(2 ** 20, 128, 512, 1024) == -3 and bp(2 ** 20, 128, 1024, 512) == -3
    assert bp(3072, 128, 512, 512, nb=0) == -3 and bp(0, 128, 512, 512) == -3
