#!/usr/bin/env python3
"""Reproducer of LAB_NOTES R7.2: on the FAST engine with a fixed timestep, discharges of -0.0 beside +0.0 come out of iteration pairs
(HP_TWO_STEP=1) with other zero signs than out of single iterations (HP_TWO_STEP=0).  Runs tests/still_pairs_worker.py fixed_negzero
both ways and prints the words whose bits differ.  HIPIMS_MI_LIB=<library> picks the build (the parent commit's shows it too).
    python tools/diag_negzero_fixed.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "still_pairs_worker.py")
res = {}
with tempfile.TemporaryDirectory() as d:
    for mode in (0, 1):
        out = os.path.join(d, f"m{mode}.npz")
        subprocess.run([sys.executable, WORKER, "fixed_negzero", out], check=True, timeout=600,
                       env=dict(os.environ, HP_TWO_STEP=str(mode), HP_PAIR_EXACT="0"))
        res[mode] = np.load(out)["state"]
a, b = res[1].view(np.uint64), res[0].view(np.uint64)
bad = np.argwhere(a != b)
print(f"words that differ: {len(bad)}")
for r, c, k in bad[:12].tolist():
    print(f"  row {r} col {c} field {k}: pairs {res[1][r, c, k]!r} single {res[0][r, c, k]!r}")
nonzero = [(r, c, k) for r, c, k in bad.tolist() if res[1][r, c, k] != 0.0 or res[0][r, c, k] != 0.0]
print(f"... of which differ by more than the sign of a zero: {len(nonzero)}")
