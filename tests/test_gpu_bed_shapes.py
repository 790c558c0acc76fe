"""The moving bed on the GPU (hp_bed_*; csrc/hp_bed.hpp).  The contract under test: an apply is exactly the host round trip it
replaces -- download state and bed, frontend.BedShapes.apply, upload the bed, upload the state -- so every comparison is
array_equal on state, bed and scalars, round by round; there are no tolerances.  Domain and runs: tests/bed_shapes_worker.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hipims_mi as hp
import bed_shapes_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(W.CASES))
def test_an_apply_is_the_round_trip(case):
    rounds, _, bed = W.compare_with_the_round_trip(case)
    for k, r in enumerate(rounds):
        print(case, k, r)
    assert all(r["same"] for r in rounds), [k for k, r in enumerate(rounds) if not r["same"]]
    assert [r["changed"] for r in rounds] == [r["want"] for r in rounds]           # bed_info's count is BedShapes.apply's, round by round
    assert all(r["t_last"] == r["t"] and r["applies"] == k + 1 for k, r in enumerate(rounds))
    ts = [r["t"] - W.T0 for r in rounds]
    assert 0.0 < ts[0] < 2.0 and ts[-1] > 14.0, ts                                 # the series begin, move and end inside the run
    assert rounds[0]["changed"] == 0 and all(r["changed"] == 0 for r in rounds if r["t"] - W.T0 <= 2.0)      # 0 before 2 s
    assert any(r["changed"] > 300 for r in rounds)                                 # the wall moves, the skipped cells do not
    after = [r for r in rounds if r["t"] - W.T0 >= 14.0]
    assert len(after) >= 2 and all(r["changed"] == 0 for r in after[1:])           # 0 from the second apply after the end on
    real = np.float64 if case.endswith("f64") else np.float32
    assert bed[50, 101] == real(0.5) and bed[0, 101] == real(9999.9) and bed[40, 101] == real(5.0)      # target; wall row and disabled cell untouched


@pytest.mark.parametrize("case", ["godunov-fast-f64", "godunov-strict-f64"])
def test_an_apply_is_the_round_trip_with_iteration_pairs(case):
    res = subprocess.run([sys.executable, os.path.join(HERE, "bed_shapes_worker.py"), case], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HP_TWO_STEP="1"))
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "identical to the round trip in every round True" in res.stdout


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_unused_is_invisible():
    a, b = W.make("godunov-fast-f64"), W.make("godunov-fast-f64")
    W.add_shapes(a)                                                                 # ... and never applied
    before = b.launch_counts()
    assert b.lib.hp_bed_apply(b.h) == 0 and b.launch_counts() == before             # no shape: HP_OK, nothing queued
    assert b.bed_info() == dict(shapes=0, cells_local=0, applies=0, changed_last=0, changed_total=0, t_last=0.0)
    for n in (7, 8, 9, 16):
        a.step_batch(n); b.step_batch(n)
    assert np.array_equal(a.download(), b.download()) and a.read_scalars() == b.read_scalars()
    assert a.launch_counts() == b.launch_counts() and a.pair_stats() == b.pair_stats()
    info = a.bed_info()
    assert info["shapes"] == 2 and info["cells_local"] == 386 and info["applies"] == 0
    with pytest.raises(hp.HipimsError, match="listed twice"):
        a.bed_shape_add([(150, 30)], 1.0, [(0.0, 0.0)])                             # another shape has it
    with pytest.raises(hp.HipimsError, match="outside the grid"):
        a.bed_shape_add([W.COLS * W.ROWS], 1.0, [(0.0, 0.0)])
    assert a.bed_info()["shapes"] == 2
    a.bed_shapes_clear(); a.bed_shapes_clear()                                      # idempotent
    assert a.bed_info()["shapes"] == 0
    a.close(); b.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint():
    dom = W.make("godunov-fast-f64")
    W.add_shapes(dom)
    batches = (7, 8)

    def rounds(lo, hi):
        out = []
        for r in range(lo, hi):
            dom.step_batch(batches[r % 2])
            dom.bed_apply()
            # (the device's scalars: cells_calculated and iterations count what the host has QUEUED, a roll-back does not take them back)
            out.append((dom.download(), dom.download(hp.ARRAY_BED), {k: v for k, v in dom.read_scalars().items() if k not in ("cells_calculated", "iterations")}))
        return out
    rounds(0, 4)                                                                    # rounds 0-3
    dom.state_save()
    first = rounds(4, 9)
    assert (first[0][1] != first[-1][1]).any()                                      # the bed moved across the rounds that are rolled back
    dom.state_restore()
    again = rounds(4, 9)
    for k, (x, y) in enumerate(zip(first, again)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2], k
    # shapes cleared since the save: the restore leaves the bed alone and says so once
    dom.state_save()
    rounds(9, 10)
    bed = dom.download(hp.ARRAY_BED)
    dom.bed_shapes_clear()
    seen = []
    hp.set_log_sink(lambda level, text: seen.append((level, text)))
    try:
        dom.state_restore()
    finally:
        hp.set_log_sink(None)
    assert len(seen) == 1 and seen[0][0] == 8 and "bed shapes were added or cleared" in seen[0][1], seen
    assert np.array_equal(dom.download(hp.ARRAY_BED), bed)
    dom.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_refused_inside_a_split_step():
    dom = W.make("godunov-fast-f64")
    W.add_shapes(dom)
    dom.step_begin()
    assert dom.lib.hp_bed_apply(dom.h) == -5 and b"between hp_step_begin and hp_step_end" in dom.lib.hp_last_error()
    dom.step_end()
    dom.bed_apply()
    assert dom.bed_info()["applies"] == 1
    dom.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,mode", [(2, "1"), (3, "1"), (2, "2"), (3, "2"), (2, "2odd")])
def test_strips(world, mode):
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", lib,
                               os.path.join(os.path.dirname(lib), "fake_rccl.cpp")])
    res = subprocess.run([sys.executable, os.path.join(HERE, "bed_strips_worker.py"), str(world), mode], capture_output=True, text=True, timeout=300)
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "FAILED" not in res.stdout and "the bed moved True" in res.stdout
