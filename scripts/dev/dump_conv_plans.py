"""Dump the forward / data-gradient conv launch queries for a fixed grid as JSON (the fixture of
tests/test_conv_plan_cpu.py, tests/golden/conv_plan_parent.json).

Only the three query bindings (conv_plan, splitk_plan, conv_pool_tp) and dispatch.override are used, so the script
runs unchanged on any commit that has them.  splitk_plan asks the device for its CU count: run it on the GPU.

    python scripts/dev/dump_conv_plans.py > tests/golden/conv_plan_parent.json

Grid: every conv of the network (forward and data gradient) at 8 x 768 x 1024, 1 x 768 x 1024, 1 x 480 x 640 (whose
1/8-resolution maps are 80 columns wide: an un-padded ragged row-ring width) and 1 x 680 x 1016 padded to a row pitch
of 1024, and every conv shape named in tests/test_gpu_conv.py and tests/test_gpu_conv_exact.py; each crossed with the
epilogues 0-7 and the dispatch variants rring x rring128 x ws64 x splitk x rring_pool.

Layout (compact: one entry per distinct answer vector): "variants" lists the dispatch variants in order; "vecs" holds
the distinct per-variant answer vectors; a "rows" entry is [N, H, W, Cin, Cout, ksize, dil, plan ids, splitk ids] with
one index into "vecs" per epilogue 0-7; a "pool_tp" entry is [Cin, Cout, ksize, tile, vec id].
"""
import ast
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

KEYS = ("rring", "rring128", "ws64", "splitk", "rring_pool")
VARIANTS = list(itertools.product((0, 1, 2), (0, 1, 2, 3), (0, 1), (0, 1), (0, 1)))
EPIS = tuple(range(8))
# (Cin, Cout, ksize, dil, resolution divisor) of the network's convs after the first layer
NET = [(64, 64, 3, 1, 1), (64, 128, 3, 1, 2), (128, 128, 3, 1, 2), (128, 256, 3, 1, 4), (256, 256, 3, 1, 4),
       (256, 512, 3, 1, 8), (512, 512, 3, 1, 8), (512, 512, 1, 1, 8), (1024, 512, 3, 2, 8), (512, 512, 3, 2, 8),
       (512, 256, 3, 2, 8), (256, 128, 3, 2, 8), (128, 64, 3, 2, 8)]
SIZES = [(8, 768, 1024), (1, 768, 1024), (1, 480, 640), (1, 680, 1024)]
POOL_TILES = (0, 11, 21, 22, 23, 25, 27, 28, 29, 31)


def test_shapes(path):
    """(n, h, w, ci, co, k, dil) of every parametrize tuple of a test file that names n, h and w."""
    out = []
    for node in ast.walk(ast.parse(open(path).read())):
        if not (isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "parametrize" and len(node.args) == 2):
            continue
        try:
            names = [s.strip() for s in ast.literal_eval(node.args[0]).split(",")]
            vals = ast.literal_eval(node.args[1])
        except (ValueError, AttributeError):
            continue
        if not {"n", "h", "w"} <= set(names):
            continue
        for v in vals:
            d = dict(zip(names, v))
            out.append((d["n"], d["h"], d["w"], d.get("ci", 64), d.get("co", 64), d.get("k", 3), d.get("dil", 1)))
    return out


def grid():
    shapes = []
    for n, h, w in SIZES:
        for ci, co, k, dil, div in NET:
            shapes.append((n, h // div, w // div, ci, co, k, dil))
    for f in ("test_gpu_conv.py", "test_gpu_conv_exact.py"):
        shapes += test_shapes(os.path.join(ROOT, "tests", f))
    both = []
    for n, h, w, ci, co, k, dil in shapes:
        if ci % 64 == 0 and co % 64 == 0:
            both += [(n, h, w, ci, co, k, dil), (n, h, w, co, ci, k, dil)]
    return sorted(set(both))


def main():
    import torch
    from can_distributed_pytorch_amd.ops import _ext, dispatch
    ext = _ext.require()
    shapes = grid()
    layers = sorted({(s[3], s[4], s[5]) for s in shapes})
    plan = {s: [[] for _ in EPIS] for s in shapes}
    splitk = {s: [[] for _ in EPIS] for s in shapes}
    tp = {(l, t): [] for l in layers for t in POOL_TILES}
    for var in VARIANTS:
        with dispatch.override(**dict(zip(KEYS, var))):
            for s in shapes:
                n, h, w, ci, co, k, dil = s
                for e in EPIS:
                    plan[s][e].append(ext.conv_plan(h, w, ci, co, k, dil, e))
                    splitk[s][e].append(ext.splitk_plan(n, h, w, ci, co, k, dil, e))
            for (ci, co, k), t in tp:
                tp[((ci, co, k), t)].append(ext.conv_pool_tp(ci, co, k, t))
    vecs, ids = [], {}

    def vid(v):
        v = tuple(v)
        if v not in ids:
            ids[v] = len(vecs)
            vecs.append(list(v))
        return ids[v]

    rows = [list(s) + [[vid(v) for v in plan[s]], [vid(v) for v in splitk[s]]] for s in shapes]
    pool = [list(l) + [t, vid(v)] for (l, t), v in sorted(tp.items())]
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    json.dump({"ncu": ncu, "keys": KEYS, "variants": VARIANTS, "vecs": vecs, "rows": rows, "pool_tp": pool},
              sys.stdout, separators=(",", ":"))
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
