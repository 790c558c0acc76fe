"""Worker of tests/test_gpu_output_stage.py::test_derive_reads_the_buffer_download_reads_and_changes_nothing (a child process:
HP_TWO_STEP is read from the environment).  Two domains run the same batches -- 1, 2, 3, 40, 41 iterations, a checkpoint, a few
iterations, the roll-back, another batch --; one of them derives all nine rasters and the statistics after every batch (and
between two batches, and right after the roll-back), the other is left alone.  Every derive must equal the host derivation of
what download() returns at that point, and the two runs must end in the same state bits and the same time.
usage: output_stage_worker.py fast|strict"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
from hipims_mi import frontend, synthetic as syn  # noqa: E402

mode = hp.MATH_STRICT if sys.argv[1] == "strict" else hp.MATH_FAST
NAMES = ["depth", "maxdepth", "fsl", "maxfsl", "dischargex", "dischargey", "velocityx", "velocityy", "froude"]
cols, rows = 512, 384
st, bed, man = syn.s_rough(cols, rows, seed=11)
calls = 0


def check(dom, where):
    global calls
    got, stats = dom.derive(NAMES), dom.stats()
    state = dom.download()
    calls += 1
    for name in NAMES:
        want = frontend.derive_output(name, state, bed, 1.0)
        if not np.array_equal(got[name], want):
            print("MISMATCH", where, name, int((got[name] != want).sum()), flush=True)
            sys.exit(1)
    wet = int(((state[..., 0] - bed > 1e-8) & (state[..., 1] > -9999.0) & (bed <= 9999.0)).sum())
    if stats["cells_wet"] != wet:
        print("MISMATCH", where, "cells_wet", stats["cells_wet"], wet, flush=True)
        sys.exit(1)


def run(watched):
    dom = hp.Domain(cols, rows, math_mode=mode)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    if watched:
        check(dom, "after upload")
    for n in (1, 2, 3, 40, 41):
        dom.step_batch(n)
        if watched:
            check(dom, f"after a batch of {n}")
    dom.state_save()
    dom.step_batch(5)
    if watched:
        check(dom, "after save + 5")
    dom.state_restore()
    if watched:
        check(dom, "after restore")
    dom.step_batch(40)
    if watched:
        check(dom, "between two batches")
    dom.step_batch(7)
    out = dom.download(), dom.read_scalars(), dom.pair_stats()["pairs"]
    dom.close()
    return out


a, sa, pairs_a = run(False)
b, sb, pairs_b = run(True)
same = np.array_equal(a.view(np.uint8), b.view(np.uint8)) and sa["time"] == sb["time"] and sa["timestep"] == sb["timestep"]
print("mode", sys.argv[1], "iteration pairs run", pairs_a, pairs_b, "derive calls", calls, "times", sa["time"], sb["time"], "same state", same, flush=True)
sys.exit(0 if same and pairs_a > 0 and pairs_b > 0 else 1)
