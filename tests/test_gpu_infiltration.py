"""The infiltration on the GPU (hp_boundary_add_infiltration; csrc/hp_soil.hpp: bdy_infiltration).  The reference is the stepwise
loop over the oracle's grid functions with frontend.Infiltration.apply on the source buffer where the engine launches
bdy_infiltration (tests/test_links.py: StepLoop; tests/test_infiltration.py: soil_scene); STRICT runs and F are compared bit for
bit, FAST fp64 at the project's FAST tolerance.  Everything runs at 40 x 32 cells."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hipims_mi as hp
import oracle
import test_infiltration as TI
import test_links as T
from hipims_mi import frontend, strips
from test_gpu_links import BATCHES, same_scalars

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
UNSUPPORTED, STATE, INVALID = -4, -5, -1


def make(math_mode=hp.MATH_STRICT, precision="f64", scheme=hp.SCHEME_GODUNOV, all_wet=False, wet_ring=False):
    st, bed, man, soil = TI.soil_scene(np.float64 if precision == "f64" else np.float32, all_wet=all_wet, wet_ring=wet_ring)
    dom = hp.Domain(T.COLS, T.ROWS, dx=T.DX, scheme=scheme, precision=precision, math_mode=math_mode)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    return dom, st, bed, man, soil


def add_rain(dom):
    dom.add_uniform(T.RAIN["definition"], T.RAIN["series"], T.RAIN["interval"], T.RAIN["length"])


def add_inflow(dom):
    dom.add_cell(T.INFLOW["depth_def"], T.INFLOW["discharge_def"], T.INFLOW["cells"], T.INFLOW["series"], T.INFLOW["interval"], T.INFLOW["length"])


def add_all(dom, soil, initial=None):
    """The rain in front of the infiltration and the cell inflow behind it."""
    add_rain(dom)
    dom.add_infiltration(soil, TI.CLASSES, initial)
    add_inflow(dom)


def raw_add(dom, soil, classes=TI.CLASSES, initial=None, class_count=None):
    """hp_boundary_add_infiltration itself: the return code."""
    ids, cls = np.ascontiguousarray(soil, np.uint8), hp.pack_soil_classes(classes)
    f0 = None if initial is None else np.ascontiguousarray(initial, np.float64)
    desc = hp.InfiltrationDesc(C.sizeof(hp.InfiltrationDesc), len(cls) if class_count is None else class_count, cls.ctypes.data, ids.ctypes.data,
                               None if f0 is None else f0.ctypes.data)
    return dom.lib.hp_boundary_add_infiltration(dom.h, C.byref(desc))


@pytest.fixture(scope="module")
def reference():
    """The reference trajectory, computed once: (state, scalars, F) after every batch."""
    assert sum(BATCHES) == 120
    st, bed, man, soil = TI.soil_scene()
    I = frontend.Infiltration(T.ROWS, T.COLS, TI.CLASSES, soil)
    loop = T.StepLoop(st, bed, man, TI.boundaries(I))
    out = []
    for n in BATCHES:
        loop.step(n)
        out.append((loop.download(), loop.scalars(), I.F.copy()))
    totals = I.branch_totals()
    assert all(totals[b] >= 1 for b in TI.REQUIRED), totals
    return out, bed


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_strict_trajectory_is_the_reference_in_every_bit(reference):
    want, _ = reference
    dom, _, _, _, soil = make(hp.MATH_STRICT)
    add_all(dom, soil)
    assert not dom.boundaries_fused() and dom.infiltration_info() == dict(classes=3, pervious_cells=int((soil != 0).sum()))
    for k, n in enumerate(BATCHES):
        dom.step_batch(n)
        state, sc, F = want[k]
        assert np.array_equal(dom.download(), state), f"state after batch {k}"
        assert same_scalars(dom.read_scalars(), sc), (k, dom.read_scalars(), sc)
        got = dom.infiltration_read()
        assert got.dtype == np.float64 and np.array_equal(got, F), (k, int((got != F).sum()), float(np.abs(got - F).max()))
    assert dom.pair_stats()["pairs"] == 0 and not dom.boundaries_fused()
    dom.close()


@pytest.mark.parametrize("scheme", [hp.SCHEME_GODUNOV, hp.SCHEME_INERTIAL], ids=["godunov", "inertial"])
def test_strict_trajectory_with_a_wet_ring_is_the_reference_in_every_bit(scheme):
    """The grid's edge ring wet, counted and pervious, and the fastest water of the domain (tests/test_infiltration.py checks that it sets the
    timestep): the engine prices the ring's part of
    the timestep once per upload, so state AND scalars equal the stepwise loop's only because the infiltration leaves the ring
    alone, as the restatement does."""
    dom, st, bed, man, soil = make(hp.MATH_STRICT, scheme=scheme, wet_ring=True)
    add_all(dom, soil)
    I = frontend.Infiltration(T.ROWS, T.COLS, TI.CLASSES, soil)
    loop = T.StepLoop(st, bed, man, TI.boundaries(I), scheme=oracle.GODUNOV if scheme == hp.SCHEME_GODUNOV else oracle.INERTIAL)
    for k, n in enumerate(BATCHES[:6]):
        dom.step_batch(n)
        loop.step(n)
        assert np.array_equal(dom.download(), loop.download()), f"state after batch {k}"
        assert same_scalars(dom.read_scalars(), loop.scalars()), (k, dom.read_scalars(), loop.scalars())
        assert np.array_equal(dom.infiltration_read(), I.F), k
    got = dom.download()
    assert np.array_equal(got[I.ring], st[I.ring]) and not I.F[I.ring].any() and I.F.max() > 1e-4
    dom.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_fast_trajectory_is_within_the_fast_tolerance(reference):
    want, bed = reference
    dom, _, _, _, soil = make(hp.MATH_FAST)
    add_all(dom, soil)
    worst = [0.0, 0.0]
    for k, n in enumerate(BATCHES):
        dom.step_batch(n)
        state, sc, F = want[k]
        got, got_f = dom.download(), dom.infiltration_read()
        inside = bed <= 9999.0
        rmse = float(np.sqrt(np.mean(((got[..., 0] - state[..., 0])[inside]) ** 2)))
        rmse_f = float(np.sqrt(np.mean(((got_f - F)[inside]) ** 2)))
        print("batch", k, "depth RMSE", rmse, "F RMSE", rmse_f)
        worst = [max(worst[0], rmse), max(worst[1], rmse_f)]
    print("largest depth RMSE", worst[0], "largest F RMSE", worst[1])
    assert worst[0] < 1e-9, worst
    assert worst[1] < 1e-9, worst
    assert dom.pair_stats()["pairs"] == 0
    dom.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math_mode", [hp.MATH_FAST, hp.MATH_STRICT], ids=["fast", "strict"])
@pytest.mark.parametrize("scheme", [hp.SCHEME_GODUNOV, hp.SCHEME_INERTIAL], ids=["godunov", "inertial"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_one_iteration_is_its_twin(precision, scheme, math_mode):
    """All wet, so that no cell is left untouched by the flux kernel: a domain with the infiltration against a fresh upload of the
    state the restatement has patched, one iteration each."""
    a, st, bed, man, soil = make(math_mode, precision, scheme, all_wet=True)
    b = make(math_mode, precision, scheme, all_wet=True)[0]
    a.add_infiltration(soil, TI.CLASSES)
    dt0 = a.read_scalars()["timestep"]
    I = frontend.Infiltration(T.ROWS, T.COLS, TI.CLASSES, soil)
    patched = st.copy()
    assert I.apply(patched, bed, dt0) >= 500 and not np.array_equal(patched, st)
    b.upload(state=patched)
    a.step_batch(1)
    b.step_batch(1)
    assert np.array_equal(a.download(), b.download())
    assert a.read_scalars() == b.read_scalars()
    got = a.infiltration_read()
    assert np.array_equal(got, I.F), (int((got != I.F).sum()), float(np.abs(got - I.F).max()))
    a.close(); b.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_infiltration_is_inert_under_muscl_hancock():
    a, st, bed, man, soil = make(hp.MATH_FAST, "f64", hp.SCHEME_MUSCL_HANCOCK, all_wet=True)
    b = make(hp.MATH_FAST, "f64", hp.SCHEME_MUSCL_HANCOCK, all_wet=True)[0]
    a.add_infiltration(soil, TI.CLASSES)
    a.step_batch(4); b.step_batch(4)
    assert np.array_equal(a.download(), b.download()) and not a.infiltration_read().any()
    a.close(); b.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_hot_start():
    """40 iterations, then a new domain from the state and F read back, time and timestep set: its next 20 iterations are the
    uninterrupted run's.  All wet -- a fresh upload fills both ping-pong buffers, and a cell the flux kernel leaves untouched would
    tell the two apart (quirk Q3) -- and without the rain, whose bursts follow the hydrological clock that no call sets."""
    a, st, bed, man, soil = make(hp.MATH_STRICT, all_wet=True)
    a.add_infiltration(soil, TI.CLASSES)
    add_inflow(a)
    a.step_batch(40)
    state, F, sc = a.download(), a.infiltration_read(), a.read_scalars()
    assert F.max() > 1e-4 and (F[soil == 0] == 0).all()
    a.step_batch(20)
    b = make(hp.MATH_STRICT, all_wet=True)[0]
    b.upload(state=state)
    b.add_infiltration(soil, TI.CLASSES, initial=F)
    add_inflow(b)
    b.set_time(sc["time"])
    b.force_timestep(sc["timestep"])
    assert np.array_equal(b.infiltration_read(), F)
    b.step_batch(20)
    sa, sb = a.read_scalars(), b.read_scalars()
    assert np.array_equal(a.download(), b.download()) and (sa["time"], sa["timestep"]) == (sb["time"], sb["timestep"])
    assert np.array_equal(a.infiltration_read(), b.infiltration_read()) and not np.array_equal(a.infiltration_read(), F)
    a.close(); b.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math_mode", [hp.MATH_FAST, hp.MATH_STRICT], ids=["fast", "strict"])
def test_save_and_restore_carry_the_cumulative_infiltration(math_mode):
    dom, _, _, _, soil = make(math_mode)
    add_all(dom, soil)
    dom.step_batch(5)
    dom.state_save()
    at_save = dom.infiltration_read()
    dom.step_batch(20)
    device = lambda sc: {k: v for k, v in sc.items() if k not in ("cells_calculated", "iterations")}      # (the host's own counts run on)
    first = (dom.download(), device(dom.read_scalars()), dom.infiltration_read())
    assert not np.array_equal(first[2], at_save)
    dom.state_restore()
    assert np.array_equal(dom.infiltration_read(), at_save)
    dom.step_batch(20)
    again = (dom.download(), device(dom.read_scalars()), dom.infiltration_read())
    assert np.array_equal(first[0], again[0]) and first[1] == again[1] and np.array_equal(first[2], again[2])
    # cleared and added again since the snapshot: F is left alone, and one warning says so
    lines = []
    hp.set_log_sink(lambda level, text: lines.append((level, text)))
    try:
        dom.clear_boundaries()
        mine = np.full((T.ROWS, T.COLS), 0.03125)
        dom.add_infiltration(soil, TI.CLASSES, initial=mine)
        dom.state_restore()
        F = dom.infiltration_read()
    finally:
        hp.set_log_sink(None)
    assert np.array_equal(F, mine)
    warnings = [text for level, text in lines if level == 8]
    assert len(warnings) == 1 and "infiltration was added or cleared" in warnings[0], lines
    dom.step_batch(3)
    assert (dom.infiltration_read() >= mine).all() and np.isfinite(dom.download()).all()
    dom.close()


# 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_strips(world):
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", lib,
                               os.path.join(os.path.dirname(lib), "fake_rccl.cpp")])
    res = subprocess.run([sys.executable, os.path.join(HERE, "infiltration_strips_worker.py"), str(world)], capture_output=True, text=True, timeout=300)
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "FAILED" not in res.stdout and "the strips are the single domain True" in res.stdout


@pytest.mark.parametrize("world", [2, 3])
def test_strip_runner_gather_infiltration(world, tmp_path):
    """StripRunner.add_infiltration / gather_infiltration themselves, with their own slicing of the global rasters: process ranks
    (torch.distributed.run) on the one GPU over the rehearsal transport, against the single domain after the same batches."""
    from test_gpu_output_stage import _torchrun
    out = os.path.join(str(tmp_path), "strips.npz")
    batches = [8, 12, 20]
    r = _torchrun(world, [os.path.join(HERE, "infiltration_rehearsal_worker.py"), out] + [str(n) for n in batches], timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = np.load(out)
    single, _, _, _, soil = make(hp.MATH_FAST)
    add_rain(single)
    f0 = TI.hot_start_raster()
    single.add_infiltration(soil, TI.CLASSES, f0)
    for n in batches:
        single.step_batch(n)
    want = single.infiltration_read()
    assert np.array_equal(got["state"], single.download()) and np.array_equal(got["F"], want)
    assert (want >= f0).all() and (want > f0).sum() > 500
    single.close()


def test_a_strip_with_two_reaches_is_unsupported_and_the_runner_gathers():
    st, bed, man, soil = TI.soil_scene()
    g = strips.ghost_rows(hp.SCHEME_GODUNOV) * 2
    own_lo, own_hi, lo, hi = strips.partition(T.ROWS, 2, g)[0]
    dom = hp.Domain(T.COLS, hi - lo, dx=T.DX, global_rows=T.ROWS, row_offset=lo, ghost_rows=g)
    dom.upload(st[lo:hi], bed[lo:hi], man[lo:hi])
    assert raw_add(dom, soil[lo:hi]) == UNSUPPORTED and "two reaches" in dom.lib.hp_last_error().decode()
    assert dom.infiltration_info() == dict(classes=0, pervious_cells=0) and not dom.boundaries_fused()
    dom.close()
    # StripRunner over the HIP engine itself (HipEngine.add_infiltration, StripRunner.gather_infiltration), one strip
    single = make(hp.MATH_STRICT)[0]
    add_rain(single)
    single.add_infiltration(soil, TI.CLASSES)
    single.step_batch(20)
    want = single.infiltration_read()
    single.close()
    runner = strips.StripRunner(T.COLS, T.ROWS, rank=0, world=1, backend="gloo", init_process_group=False, loop="torch", exchange_period=1,
                                dx=T.DX, math_mode=hp.MATH_STRICT)
    runner.upload_global(st, bed, man)
    runner.set_target_time(1e9)
    add_rain(runner.domain)
    runner.add_infiltration(soil, TI.CLASSES)
    runner.domain.step_batch(20)
    got = runner.gather_infiltration()
    assert got.dtype == np.float64 and np.array_equal(got, want) and want.max() > 0
    runner.engine.close()


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_clear_removes_it_and_a_bare_domain_queues_what_it_did():
    a, st, bed, man, soil = make(hp.MATH_FAST, all_wet=True)
    b = make(hp.MATH_FAST, all_wet=True)[0]
    a.add_infiltration(soil, TI.CLASSES)
    assert a.infiltration_info()["classes"] == 3 and not a.boundaries_fused()
    a.clear_boundaries()
    assert a.infiltration_info() == dict(classes=0, pervious_cells=0)
    raster = np.zeros((T.ROWS, T.COLS))
    assert a.lib.hp_infiltration_read(a.h, raster.ctypes.data, 0, T.ROWS) == STATE
    with pytest.raises(hp.HipimsError):
        a.infiltration_read()
    for dom in (a, b):
        add_rain(dom)
    counts = (a.launch_counts(), b.launch_counts())
    a.step_batch(20); b.step_batch(20)
    assert np.array_equal(a.download(), b.download()) and a.read_scalars() == b.read_scalars()
    assert a.boundaries_fused() == b.boundaries_fused()
    la, lb = a.launch_counts(), b.launch_counts()
    assert (la[0] - counts[0][0], la[1] - counts[0][1]) == (lb[0] - counts[1][0], lb[1] - counts[1][1])
    assert a.pair_stats()["pairs"] == b.pair_stats()["pairs"]
    a.add_infiltration(soil, TI.CLASSES)                  # a second add works once the first is gone
    a.step_batch(2)
    assert a.infiltration_read().max() > 0
    a.close(); b.close()


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_through_the_abi():
    dom, _, _, _, soil = make(hp.MATH_FAST)
    lib = dom.lib
    last = lambda: lib.hp_last_error().decode()
    assert lib.hp_boundary_add_infiltration(dom.h, None) == INVALID and "NULL" in last()
    assert lib.hp_boundary_add_infiltration(None, None) == INVALID
    wrong = soil.copy()
    wrong[7, 9] = 4
    assert raw_add(dom, wrong) == INVALID and f"cell {7 * T.COLS + 9} " in last()
    for name, (cls, word) in TI.BAD_CLASSES.items():
        assert raw_add(dom, soil % 3, [TI.GOOD_CLASS, cls]) == INVALID and word in last(), (name, last())
    assert raw_add(dom, soil, class_count=0) == INVALID and raw_add(dom, soil, TI.CLASSES * 85, class_count=256) == INVALID
    f0 = np.zeros((T.ROWS, T.COLS))
    f0[2, 5] = -1.0
    assert raw_add(dom, soil, initial=f0) == INVALID and f"cell {2 * T.COLS + 5}:" in last()
    assert dom.infiltration_info() == dict(classes=0, pervious_cells=0)
    dom.step_begin()
    assert raw_add(dom, soil) == STATE                    # inside a split step
    dom.step_end()
    assert raw_add(dom, soil) == 0
    assert raw_add(dom, soil) == STATE and "already" in last()           # a second add
    raster = np.zeros((T.ROWS + 1, T.COLS))
    for row0, nrows in ((0, T.ROWS + 1), (-1, 2), (T.ROWS, 1), (3, -1)):
        assert lib.hp_infiltration_read(dom.h, raster.ctypes.data, row0, nrows) == INVALID, (row0, nrows)
    assert lib.hp_infiltration_read(dom.h, None, 0, 1) == INVALID
    dom.step_begin()
    assert lib.hp_infiltration_read(dom.h, raster.ctypes.data, 0, 1) == STATE
    dom.step_end()
    # the domain is as usable as before
    dom.step_batch(5)
    assert np.array_equal(dom.infiltration_read(row0=4, nrows=3), dom.infiltration_read()[4:7]) and np.isfinite(dom.download()).all()
    dom.close()
