"""The tracer on the GPU (hp_tracer_enable; csrc/hp_tracer.hpp: tracer_sources, tracer_step).  The reference is the stepwise loop
over the oracle's grid functions with frontend.Tracer.apply behind the boundaries and in front of the flux step, where the engine
launches the two kernels (tests/test_links.py: StepLoop; tests/test_tracer.py: TracedLoop); M is compared bit for bit everywhere,
in FAST arithmetic too: the tracer's face solve is the exact one whatever the math mode.  Everything runs at 40 x 32 cells or
smaller."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hipims_mi as hp
import test_infiltration as TI
import test_links as T
import test_tracer as TT
from hipims_mi import frontend, strips
from test_gpu_infiltration import raw_add
from test_gpu_links import same_scalars

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
UNSUPPORTED, STATE, INVALID = -4, -5, -1
BATCHES = [1, 3, 7, 1, 3, 7, 1, 3, 7, 7]                 # 40 iterations in batches of 1, 3 and 7
REAL = dict(f64=np.float64, f32=np.float32)


def make(math_mode=hp.MATH_STRICT, precision="f64", scheme=hp.SCHEME_GODUNOV):
    st, bed, man, _ = T.scene(REAL[precision])
    dom = hp.Domain(T.COLS, T.ROWS, dx=T.DX, scheme=scheme, precision=precision, math_mode=math_mode)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    return dom, st, bed, man


def add_rain(dom):
    dom.add_uniform(T.RAIN["definition"], T.RAIN["series"], T.RAIN["interval"], T.RAIN["length"])


def add_inflow(dom):
    dom.add_cell(T.INFLOW["depth_def"], T.INFLOW["discharge_def"], T.INFLOW["cells"], T.INFLOW["series"], T.INFLOW["interval"], T.INFLOW["length"])


def raw_enable(dom, initial=None, struct_size=None):
    """hp_tracer_enable itself: the return code."""
    m0 = None if initial is None else np.ascontiguousarray(initial, np.float64)
    desc = hp.TracerDesc(C.sizeof(hp.TracerDesc) if struct_size is None else struct_size, 0, None if m0 is None else m0.ctypes.data)
    return dom.lib.hp_tracer_enable(dom.h, C.byref(desc))


def differing(got, want):
    return int((got != want).sum()), float(np.abs(got - want).max())


@pytest.fixture(scope="module", params=["f64", "f32"])
def reference(request):
    """The reference trajectory of one precision, computed once: (state, scalars, M) after every batch."""
    precision = request.param
    st, bed, man, _ = T.scene(REAL[precision])
    tr = frontend.Tracer(T.ROWS, T.COLS, T.DX, TT.functions(precision), initial=TT.blob())
    tr.add_source(TT.SOURCE["cells"], TT.SOURCE["series"])
    loop = TT.TracedLoop(st, bed, man, tr, boundaries=[("uniform", T.RAIN), ("cell", T.INFLOW)], precision=precision)
    out = []
    for n in BATCHES:
        loop.step(n)
        out.append((loop.download(), loop.scalars(), tr.M.copy()))
    totals = tr.branch_totals()
    assert all(totals[b] > 0 for b in ("ring", "disabled", "moved", "source", "no_concentration", "e_pos", "e_neg", "n_pos", "s_neg")), totals
    return precision, out


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_strict_trajectory_is_the_reference_in_every_bit(reference):
    """Rain, a cell inflow and one tracer source; the tracer is enabled BEFORE the boundaries are added and still steps behind them."""
    precision, want = reference
    dom = make(hp.MATH_STRICT, precision)[0]
    dom.tracer_enable(TT.blob())
    dom.tracer_add_source(TT.SOURCE["cells"], TT.SOURCE["series"])
    add_rain(dom)
    add_inflow(dom)
    assert not dom.boundaries_fused() and dom.tracer_info() == dict(iterations=0, sources=1, source_cells=3)
    launches = dom.launch_counts()[0]
    for k, n in enumerate(BATCHES):
        dom.step_batch(n)
        state, sc, M = want[k]
        assert np.array_equal(dom.download(), state), f"state after batch {k}"
        assert same_scalars(dom.read_scalars(), sc), (k, dom.read_scalars(), sc)
        got = dom.tracer_read()
        assert got.dtype == np.float64 and np.array_equal(got, M), (k,) + differing(got, M)
    assert dom.launch_counts()[0] - launches == 40 and dom.pair_stats()["pairs"] == 0        # one flux launch an iteration: no pair
    assert dom.tracer_info()["iterations"] == 40 and not np.array_equal(dom.tracer_read(), TT.blob())
    dom.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_fast_iterations_move_the_tracer_by_the_exact_face_solve():
    """FAST fp64, no boundaries, batches of one iteration: M after each equals frontend.Tracer on exactly the state and the
    timestep the iteration started from.  One arithmetic whatever the math mode."""
    dom, _, bed, _ = make(hp.MATH_FAST)
    dom.tracer_enable(TT.blob())
    dom.tracer_add_source(TT.SOURCE["cells"], TT.SOURCE["series"])
    tr = frontend.Tracer(T.ROWS, T.COLS, T.DX, TT.functions("f64"), initial=TT.blob())
    tr.add_source(TT.SOURCE["cells"], TT.SOURCE["series"])
    for k in range(8):
        state, sc = dom.download(), dom.read_scalars()
        dom.step_batch(1)
        assert tr.apply(state, bed, sc["timestep"], sc["time"]) > 1000
        got = dom.tracer_read()
        assert np.array_equal(got, tr.M), (k,) + differing(got, tr.M)
    assert dom.pair_stats()["pairs"] == 0 and not np.array_equal(tr.M, TT.blob())
    dom.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("cols,rows", [(5, 5), (67, 9), (130, 6)], ids=["5x5", "67x9", "130x6"])
def test_widths_at_the_wave_edges(cols, rows, precision):
    """A partial wave, 64 + 3 columns and three waves a row: a tilted wet surface over a rough bed, random M >= 0, one iteration."""
    rng = np.random.default_rng(cols * 100 + rows)
    real = REAL[precision]
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    bed = np.round(0.2 * rng.random((rows, cols)), 4)
    st = np.zeros((rows, cols, 4))
    st[..., 0] = 1.0 + 0.004 * x - 0.01 * y
    st[..., 2] = np.round(0.1 * rng.standard_normal((rows, cols)), 4)
    st[..., 3] = np.round(0.1 * rng.standard_normal((rows, cols)), 4)
    st[..., 1] = st[..., 0]
    st, bed, man = st.astype(real), bed.astype(real), np.full((rows, cols), 0.03, real)
    m0 = rng.random((rows, cols)) * (rng.random((rows, cols)) > 0.2)
    dom = hp.Domain(cols, rows, dx=1.0, precision=precision, math_mode=hp.MATH_STRICT)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.tracer_enable(m0)
    sc = dom.read_scalars()
    dom.step_batch(1)
    tr = frontend.Tracer(rows, cols, 1.0, TT.functions(precision, dx=1.0), initial=m0)
    assert tr.apply(st, bed, sc["timestep"], sc["time"]) == (cols - 2) * (rows - 2)
    got = dom.tracer_read()
    assert np.array_equal(got, tr.M), differing(got, tr.M)
    assert not np.array_equal(got[1:-1, 1:-1], m0[1:-1, 1:-1]) and np.array_equal(got[0], m0[0]) and np.array_equal(got[:, -1], m0[:, -1])
    dom.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,precision", [("fast", "f64"), ("strict", "f32")])
def test_the_traced_run_is_the_untraced_run(mode, precision):
    """The switch that holds the untraced run to single iterations is read once per process: a process of its own."""
    res = subprocess.run([sys.executable, os.path.join(HERE, "tracer_untraced_worker.py"), mode, precision], capture_output=True, text=True, timeout=120)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "the traced run is the untraced run True" in res.stdout


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math_mode", [hp.MATH_FAST, hp.MATH_STRICT], ids=["fast", "strict"])
def test_save_and_restore_carry_the_tracer(math_mode):
    dom = make(math_mode)[0]
    add_rain(dom)
    add_inflow(dom)
    dom.tracer_enable(TT.blob())
    dom.tracer_add_source(TT.SOURCE["cells"], TT.SOURCE["series"])
    dom.step_batch(5)                                     # an odd number: the checkpoint's M lies in the second buffer
    dom.state_save()
    at_save = dom.tracer_read()
    dom.step_batch(10)
    device = lambda sc: {k: v for k, v in sc.items() if k not in ("cells_calculated", "iterations")}      # (the host's own counts run on)
    first = (dom.download(), device(dom.read_scalars()), dom.tracer_read())
    assert not np.array_equal(first[2], at_save) and dom.tracer_info()["iterations"] == 15
    dom.state_restore()
    assert np.array_equal(dom.tracer_read(), at_save) and dom.tracer_info()["iterations"] == 5
    dom.step_batch(10)
    again = (dom.download(), device(dom.read_scalars()), dom.tracer_read())
    assert np.array_equal(first[0], again[0]) and first[1] == again[1] and np.array_equal(first[2], again[2])
    dom.close()


def test_enabling_after_the_save_leaves_the_tracer_alone_with_a_warning():
    dom = make(hp.MATH_FAST)[0]
    add_inflow(dom)                                       # (the scene's water is at rest without it, and M with it)
    dom.step_batch(3)
    dom.state_save()
    lines = []
    hp.set_log_sink(lambda level, text: lines.append((level, text)))
    try:
        mine = TT.blob() + 0.03125
        dom.tracer_enable(mine)
        dom.step_batch(4)
        moved = dom.tracer_read()
        dom.state_restore()
        M = dom.tracer_read()
    finally:
        hp.set_log_sink(None)
    assert np.array_equal(M, moved) and not np.array_equal(moved, mine)
    warnings = [text for level, text in lines if level == 8]
    assert len(warnings) == 1 and "tracer was enabled or disabled" in warnings[0], lines
    dom.step_batch(3)
    assert np.isfinite(dom.tracer_read()).all() and np.isfinite(dom.download()).all()
    dom.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_write_then_read_round_trips_a_row_range():
    dom = make(hp.MATH_FAST)[0]
    dom.tracer_enable(TT.blob())
    rows = np.random.default_rng(5).random((7, T.COLS))
    dom.tracer_write(rows, row0=11)
    assert np.array_equal(dom.tracer_read(row0=11, nrows=7), rows)
    want = TT.blob()
    want[11:18] = rows
    assert np.array_equal(dom.tracer_read(), want)
    # ... and what was written is what the next iteration moves
    state, sc, bed = dom.download(), dom.read_scalars(), dom.download(hp.ARRAY_BED)
    tr = frontend.Tracer(T.ROWS, T.COLS, T.DX, TT.functions("f64"), initial=want)
    dom.step_batch(1)
    tr.apply(state, bed, sc["timestep"], sc["time"])
    assert np.array_equal(dom.tracer_read(), tr.M)
    # hp_domain_upload and hp_boundary_clear do not touch M
    before = dom.tracer_read()
    dom.upload(state=state)
    add_rain(dom)
    dom.clear_boundaries()
    assert np.array_equal(dom.tracer_read(), before) and dom.tracer_info()["iterations"] == 1
    raster = np.zeros((T.ROWS + 1, T.COLS))
    for row0, nrows in ((0, T.ROWS + 1), (-1, 2), (T.ROWS, 1), (3, -1)):
        assert dom.lib.hp_tracer_read(dom.h, raster.ctypes.data, row0, nrows) == INVALID, (row0, nrows)
        assert dom.lib.hp_tracer_write(dom.h, raster.ctypes.data, row0, nrows) == INVALID, (row0, nrows)
    assert dom.lib.hp_tracer_read(dom.h, None, 0, 1) == INVALID and dom.lib.hp_tracer_write(dom.h, None, 0, 1) == INVALID
    dom.step_begin()
    assert dom.lib.hp_tracer_read(dom.h, raster.ctypes.data, 0, 1) == STATE and dom.lib.hp_tracer_write(dom.h, raster.ctypes.data, 0, 1) == STATE
    assert raw_enable(dom) == STATE
    dom.step_end()
    dom.tracer_disable()
    assert dom.lib.hp_tracer_read(dom.h, raster.ctypes.data, 0, 1) == STATE and dom.tracer_info() == dict(iterations=0, sources=0, source_cells=0)
    dom.tracer_disable()                                  # idempotent
    dom.close()


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    last = lambda dom: dom.lib.hp_last_error().decode()
    # a scheme other than Godunov
    for scheme in (hp.SCHEME_MUSCL_HANCOCK, hp.SCHEME_INERTIAL):
        dom = make(hp.MATH_FAST, scheme=scheme)[0]
        assert raw_enable(dom) == UNSUPPORTED and "Godunov" in last(dom)
        assert dom.tracer_info() == dict(iterations=0, sources=0, source_cells=0)
        dom.step_batch(2)
        dom.close()
    # a strip descriptor
    st, bed, man, links = T.scene()
    g = strips.ghost_rows(hp.SCHEME_GODUNOV)
    own_lo, own_hi, lo, hi = strips.partition(T.ROWS, 2, g)[0]
    dom = hp.Domain(T.COLS, hi - lo, dx=T.DX, global_rows=T.ROWS, row_offset=lo, ghost_rows=g)
    dom.upload(st[lo:hi], bed[lo:hi], man[lo:hi])
    assert raw_enable(dom) == UNSUPPORTED and "strip" in last(dom)
    dom.close()
    # a domain with links, a domain with an infiltration
    soil = TI.soil_scene()[3]
    packed = hp.pack_links(links, T.COLS)
    dom = make()[0]
    dom.add_links(links)
    assert raw_enable(dom) == UNSUPPORTED and "link" in last(dom)
    dom.close()
    dom = make()[0]
    dom.add_infiltration(soil, TI.CLASSES)
    assert raw_enable(dom) == UNSUPPORTED and "infiltration" in last(dom)
    dom.close()
    # ... and the reverse orders
    dom = make()[0]
    assert raw_enable(dom, TT.blob()) == 0
    assert dom.lib.hp_boundary_add_links(dom.h, packed.ctypes.data, len(packed)) == UNSUPPORTED and "tracer" in last(dom)
    assert raw_add(dom, soil) == UNSUPPORTED and "tracer" in last(dom)
    assert dom.links_info()["links"] == 0 and dom.infiltration_info() == dict(classes=0, pervious_cells=0)
    assert raw_enable(dom) == STATE and "already" in last(dom)                  # a second enable
    # argument errors through the ABI, before any device call
    bad = TT.blob()
    bad[2, 5] = -1.0
    assert raw_enable(dom, bad) == INVALID and f"cell {2 * T.COLS + 5}:" in last(dom)
    assert raw_enable(dom, struct_size=12) == INVALID and dom.lib.hp_tracer_enable(dom.h, None) == INVALID
    cells, series = np.array([9 * T.COLS + 9], np.uint64), np.array([(0.0, 1.0)])
    add = lambda c, s: dom.lib.hp_tracer_add_source(dom.h, c.ctypes.data, len(c), s.ctypes.data, len(s))
    assert add(np.array([5], np.uint64), series) == INVALID and "edge ring" in last(dom)
    assert add(cells, np.array([(0.0, 1.0), (0.0, 2.0)])) == INVALID and "strictly increasing" in last(dom)
    assert add(cells, series) == 0 and add(cells, series) == INVALID and "listed twice" in last(dom)
    dom.tracer_sources_clear()
    assert dom.tracer_info()["sources"] == 0 and add(cells, series) == 0
    # hp_bed_apply keeps the depth and so leaves M alone: the combination is allowed
    dom.bed_shape_add([(30, 10), (31, 10)], [0.6, 0.6], [(0.0, 0.0), (1.0, 1.0)])
    dom.step_batch(3)
    before = dom.tracer_read()
    dom.bed_apply()
    assert np.array_equal(dom.tracer_read(), before)
    dom.step_batch(3)
    assert np.isfinite(dom.tracer_read()).all()
    dom.close()


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_model_writes_the_concentration(tmp_path):
    from hipims_mi.model import Model
    xml, m0 = TT.write_model(tmp_path)
    m = Model(xml, output_format=".npy")
    assert m.sim.tracer_info() == dict(iterations=0, sources=1, source_cells=2)
    m.run()
    M = m.sim.tracer_read()
    assert np.array_equal(np.load(tmp_path / "out" / "tracer_2.npy"), M) and M[3, 3] > 0 and M[3, 4] > 0 and m0[3, 3] == 0
    assert np.array_equal(np.load(tmp_path / "out" / "conc_2.npy"), frontend.tracer_concentration(M, m.sim.download(), m.bed))
    assert m.sim.tracer_info()["iterations"] > 0
    m.sim.close()
