"""Skipped tiles in the FAST fp64 pair kernel (hp_kernels.hpp: godunov_march2, StillRec; round 8): a tile whose whole stencil the
launch before recorded as one still state, found as it left it, is neither loaded nor stored.  That must change no bit, so every case
holds the default run to the same run without the skip (HP_PAIR_SKIP=0) and, where the two already agree, to single iterations
(HP_TWO_STEP=0) -- as bit patterns, so that a -0.0 discharge counts.  Every case also checks that tiles were skipped
(hp_pair_stats out[9])."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
WORKER = os.path.join(HERE, "pair_skip_worker.py")


def run(case, tmp_path, two_step, skip):
    out = os.path.join(str(tmp_path), f"{case}_{two_step}_{skip}.npz")
    r = subprocess.run([sys.executable, WORKER, case, out], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, HP_TWO_STEP=str(two_step), HP_PAIR_SKIP=str(skip), HP_PAIR_EXACT="0"))
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


def same_bits(a, b, what):
    assert int(a["iterations"]) == int(b["iterations"]), what
    assert a["t"].view(np.uint64) == b["t"].view(np.uint64), what
    assert a["dt"].view(np.uint64) == b["dt"].view(np.uint64), what
    x, y = a["state"].view(np.uint64), b["state"].view(np.uint64)
    assert x.shape == y.shape
    bad = np.argwhere(x != y)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[:5].tolist()}"


# negzero_fixed: against HP_PAIR_SKIP=0 only -- pairs and single iterations already part there (LAB_NOTES R7.2)
@pytest.mark.parametrize("case", ["dam", "dam_fixed", "fronts", "ulp", "zmax", "negzero", "negzero_fixed", "disabled", "interleave"])
def test_skipped_tiles_change_no_bit(case, tmp_path):
    skip, full = run(case, tmp_path, 1, 1), run(case, tmp_path, 1, 0)
    # pairs were taken (interleave: its odd batches, restore, upload and clipped steps run single iterations too)
    assert int(skip["launches"]) < int(skip["iterations"]) * (0.8 if case == "interleave" else 0.62)
    assert int(skip["skipped"].max()) > 0, skip["skipped"].tolist()             # ... and tiles skipped
    assert int(full["skipped"].max()) == 0                                      # HP_PAIR_SKIP=0 skips nothing
    same_bits(skip, full, "HP_PAIR_SKIP=0")
    if case != "negzero_fixed":
        same_bits(skip, run(case, tmp_path, 0, 1), "single iterations")
