"""usage: cmp_bytes.py PARENT_DIR NEW_DIR -- compare the dumped files of the two arms byte for byte (synth gt / dmax also
at the tolerance of tests/test_gpu_components.py::test_synthetic_gpu_generator)."""
import hashlib
import os
import sys

import numpy as np

A, B = sys.argv[1], sys.argv[2]
na, nb = sorted(os.listdir(A)), sorted(os.listdir(B))
bad = 0
if na != nb:
    print("FILE LISTS DIFFER:", sorted(set(na) ^ set(nb)))
    bad += 1
print(f"| file | bytes | sha256 (first 12) | verdict |\n|---|---|---|---|")
for f in na:
    if f not in nb:
        continue
    a, b = open(os.path.join(A, f), "rb").read(), open(os.path.join(B, f), "rb").read()
    same = a == b
    verdict = "identical" if same else "DIFFERENT"
    if not same and f.startswith(("synth_gt", "synth_dmax")) and len(a) == len(b):
        close = np.allclose(np.frombuffer(a, np.float32), np.frombuffer(b, np.float32), rtol=1e-5, atol=1e-6)
        verdict = "within rtol 1e-5 / atol 1e-6" if close else "DIFFERENT"
        same = close
    bad += not same
    print(f"| {f} | {len(a)} | {hashlib.sha256(b).hexdigest()[:12]} | {verdict} |")
print(f"\n{len(na)} files compared, {bad} mismatches: " + ("ALL IDENTICAL" if not bad else "MISMATCH"))
sys.exit(1 if bad else 0)
