#!/usr/bin/env python3
"""Records tests/golden/kernarg_order.npz on the GPU: what optimize(4) returns for every case of tests/kernarg_order_cases.py
in graph-replay mode (chi2 and robust chi2 of every iterate, PCG iteration counts, final poses).  To be run at the commit
BEFORE a change of the kernels' parameter lists; tests/test_gpu_kernarg_order.py then asks for the same bits.
    python scripts/make_golden_kernarg_order.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kernarg_order_cases as kc  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "kernarg_order.npz")
rec = {}
for name in kc.CASES:
    r = rec[name] = kc.run(name, dict(kc.MODES)["graph"])
    print(name, "chi2", [float(f"{c:.6g}") for c in r["chi2"]], "pcg", r["pcg_iters"].tolist())
kc.save(out, rec)
print(out, os.path.getsize(out), "bytes")
