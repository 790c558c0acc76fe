"""Still runs in the FAST fp64 pair kernel (hp_kernels.hpp: godunov_march2, still_run): a tile that starts in still water is marched
by loads and stores alone until a row breaks the run.  That must be the same computation as the full march, so the engine with
pairs (HP_TWO_STEP=1) is held to single iterations (HP_TWO_STEP=0, godunov_march, which has no such shortcut in FAST) BIT FOR
BIT -- as bit patterns: a discharge of -0.0 counts as at rest, and -0.0 == 0.0 would hide a sign the shortcut got wrong.  The
exact flavour (HP_PAIR_EXACT=1) does not take still runs and stays under tests/test_gpu_two_step.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
WORKER = os.path.join(HERE, "still_pairs_worker.py")


def run(variant, tmp_path, mode):
    out = os.path.join(str(tmp_path), f"{variant}_{mode}.npz")
    r = subprocess.run([sys.executable, WORKER, variant, out], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, HP_TWO_STEP=str(mode), HP_PAIR_EXACT="0"))
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


@pytest.mark.parametrize("variant", ["dynamic", "fixed", "lake"])
def test_still_runs_are_the_same_computation_as_single_iterations(variant, tmp_path):
    single, pairs = run(variant, tmp_path, 0), run(variant, tmp_path, 1)
    assert int(pairs["launches"]) < int(pairs["iterations"]) * 0.62             # pairs were taken
    assert int(pairs["iterations"]) == int(single["iterations"])
    assert pairs["t"].view(np.uint64) == single["t"].view(np.uint64)
    assert pairs["dt"].view(np.uint64) == single["dt"].view(np.uint64)
    a, b = pairs["state"].view(np.uint64), single["state"].view(np.uint64)
    assert a.shape == b.shape
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"{len(bad)} words differ, first at {bad[:5].tolist()}"


def test_still_runs_in_row_strips_with_peer_ghost_rows():
    """TAIL 2: three row strips as threads on one GPU, two reaches of ghost rows written into the neighbours by the pair kernel."""
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", lib,
                               os.path.join(os.path.dirname(lib), "fake_rccl.cpp")])
    r = subprocess.run([sys.executable, os.path.join(HERE, "still_strips_worker.py")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, HP_TWO_STEP="1", HP_PAIR_EXACT="0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bit-identical True" in r.stdout
