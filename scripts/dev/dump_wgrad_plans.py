"""Dump the weight-gradient planner's answers for a fixed grid as JSON (the fixture of tests/test_wgrad_plan_cpu.py,
tests/golden/wgrad_plan_parent.json).

Only wgrad_plan, WgradWorkspace.plan, wgrad_1x1_batched_plan and dispatch.override are used, so the script runs
unchanged on any commit that has them.  Without a device the planner assumes 256 CUs (an MI355X's count), so the dump
may be made on a machine without a GPU; "ncu" records the count the answers hold for.

    python scripts/dev/dump_wgrad_plans.py > tests/golden/wgrad_plan_parent.json

Grid: the shape grid of dump_conv_plans.py (every conv of the network at its four input sizes and every conv shape
named in tests/test_gpu_conv.py and tests/test_gpu_conv_exact.py, both channel orders) and the first layer at the four
sizes and the two first-layer test shapes; each crossed with dispatch wgrad_tap 0-3 and the map width given / unknown
(W = 0).  The batched 1x1 plan: M of the four sizes' 1/8-resolution maps and of the test shape, ncu 128 / 192 / 224 /
256.

Layout (one entry per distinct answer vector): "vecs" holds the distinct vectors of 8 answers [S, mslice, cfg, need],
ordered wgrad_tap 0-3 x (W given, W = 0); a "rows" entry is [N, H, W, Cin, Cout, ksize, dil, first, vec id]; a
"batched" entry is [M, nb, Cin, Cout, ncu, S, mslice, need].
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dump_conv_plans import SIZES, grid  # noqa: E402

FIRST_TEST_SHAPES = [(2, 40, 56), (1, 9, 13)]
TAPS = (0, 1, 2, 3)
BATCHED_TEST_M = 2 * 12 * 128
BATCHED_NCU = (128, 192, 224, 256)


def queries():
    """(n, h, w, ci, co, k, dil, first) of the grid."""
    out = [s + (0,) for s in grid()]
    out += [(n, h, w, 4, 64, 3, 1, 1) for n, h, w in SIZES + FIRST_TEST_SHAPES]
    return out


def main():
    import torch
    from can_distributed_pytorch_amd.ops import _ext, dispatch
    from can_distributed_pytorch_amd.ops import conv as C
    ext = _ext.require()
    ws = C.WgradWorkspace("cpu")
    vecs, ids, rows = [], {}, []
    qs = queries()
    answers = {q: [] for q in qs}
    for tap in TAPS:
        with dispatch.override(wgrad_tap=tap):
            for q in qs:
                n, h, w, ci, co, k, dil, first = q
                for wq in (w, 0):
                    a = ws.plan(n * h * w, ci, co, k, bool(first), dil, wq)
                    assert tuple(a[:3]) == tuple(ext.wgrad_plan(n * h * w, ci, co, k, first, 1024, dil, wq)), q
                    answers[q].append([int(v) for v in a])
    for q in qs:
        v = tuple(map(tuple, answers[q]))
        if v not in ids:
            ids[v] = len(vecs)
            vecs.append(answers[q])
        rows.append(list(q) + [ids[v]])
    batched = []
    for m in sorted({n * (h // 8) * (w // 8) for n, h, w in SIZES} | {BATCHED_TEST_M}):
        for ncu in BATCHED_NCU:
            batched.append([m, 4, 512, 512, ncu] + [int(v) for v in C.wgrad_1x1_batched_plan(m, 4, 512, 512, ncu=ncu)])
    ncu = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    json.dump({"ncu": ncu, "taps": TAPS, "vecs": vecs, "rows": rows, "batched": batched}, sys.stdout,
              separators=(",", ":"))
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
