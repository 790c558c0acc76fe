"""The tracer set on the GPU (hp_tracer_enable_set; csrc/hp_tracer.hpp: tracer_sources, tracer_step_set).  Two references: the single
tracer of the same build (hp_tracer_enable, tracer_step), which species s of a set must equal in every bit when it does not decay,
and frontend.TracerSet, the NumPy restatement with step 6.  Every comparison is array_equal; everything runs at 40 x 32 cells or
smaller, but for the 130- and 67-column shapes of the wave-edge cases."""
import ctypes as C

import numpy as np
import pytest

import hipims_mi as hp
import test_infiltration as TI
import test_links as T
import test_tracer as TT
import test_tracer_set as TS
from hipims_mi import frontend, strips
from test_gpu_infiltration import raw_add
from test_gpu_tracer import BATCHES, INVALID, REAL, STATE, UNSUPPORTED, add_inflow, add_rain, differing, make

pytestmark = pytest.mark.gpu
LAMBDAS = (0.0, 1e-6, 1e-3, 0.1, 1.0, 10.0, 1e3, 0.0)


def raw_enable_set(dom, species, decay=None, initial=None, struct_size=None):
    """hp_tracer_enable_set itself: the return code."""
    lam = None if decay is None else np.ascontiguousarray(decay, np.float64)
    m0 = None if initial is None else np.ascontiguousarray(initial, np.float64)
    desc = hp.TracerSetDesc(C.sizeof(hp.TracerSetDesc) if struct_size is None else struct_size, species, None if lam is None else lam.ctypes.data,
                            None if m0 is None else m0.ctypes.data)
    return dom.lib.hp_tracer_enable_set(dom.h, C.byref(desc))


def read_all(dom, species):
    return np.stack([dom.tracer_read(species=s) for s in range(species)])


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("math_mode", [hp.MATH_FAST, hp.MATH_STRICT], ids=["fast", "strict"])
def test_a_set_is_that_many_single_tracers(math_mode, precision):
    """Three species without decay -- the blob, zeros, a gradient -- with sources on species 0 and 2 (one cell in both), rain and the
    cell inflow: after every batch each plane is the M of a hp_tracer_enable run of that species alone, and the water, the scalars,
    the launch counts and the pair statistics are that run's."""
    M0 = TS.planes()
    sources = {0: TT.SOURCE, 2: TS.SOURCE_2}

    # the set, its planes after every batch
    dom = make(math_mode, precision)[0]
    dom.tracer_enable_set(initial=M0)
    for s, src in sources.items():
        dom.tracer_add_source(src["cells"], src["series"], species=s)
    add_rain(dom)
    add_inflow(dom)
    assert dom.tracer_set_info() == dict(species=3, decay=[0.0, 0.0, 0.0]) and dom.tracer_info() == dict(iterations=0, sources=2, source_cells=5)
    assert not dom.boundaries_fused()
    got = []
    for n in BATCHES:
        dom.step_batch(n)
        got.append((dom.download(), dom.read_scalars(), read_all(dom, 3)))
    set_counts, set_pairs = dom.launch_counts(), dom.pair_stats()["pairs"]
    assert dom.tracer_info()["iterations"] == sum(BATCHES)
    dom.close()
    for s in range(3):
        single = make(math_mode, precision)[0]
        single.tracer_enable(M0[s])
        if s in sources:
            single.tracer_add_source(sources[s]["cells"], sources[s]["series"])
        add_rain(single)
        add_inflow(single)
        for k, n in enumerate(BATCHES):
            single.step_batch(n)
            M = single.tracer_read()
            assert np.array_equal(got[k][2][s], M), (s, k) + differing(got[k][2][s], M)
            assert np.array_equal(got[k][0], single.download()) and got[k][1] == single.read_scalars(), (s, k)
        assert single.launch_counts() == set_counts and single.pair_stats()["pairs"] == set_pairs == 0
        single.close()
    assert not got[-1][2][1].any() and not np.array_equal(got[-1][2][0], M0[0]) and not np.array_equal(got[-1][2][2], M0[2])


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_eight_decaying_species_equal_the_restatement(precision):
    """STRICT, batches of one iteration: water set in motion by the inflow, which is then cleared (the restatement is handed the
    downloaded state, and a boundary would change it in front of the tracer); a target time the run reaches, so that the last
    iterations are suspended.  Every plane equals frontend.TracerSet.apply on the state and the timestep the iteration started from."""
    real = REAL[precision]
    st, bed, man = (a.astype(real) for a in TT.traced_scene())
    dom = hp.Domain(T.COLS, T.ROWS, dx=T.DX, precision=precision, math_mode=hp.MATH_STRICT)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    add_inflow(dom)
    dom.step_batch(6)
    dom.clear_boundaries()
    rng = np.random.default_rng(8)
    M0 = np.stack([TT.blob() * (s + 1) + (rng.random((T.ROWS, T.COLS)) < 0.3) * rng.random((T.ROWS, T.COLS)) for s in range(8)])
    dom.tracer_enable_set(initial=M0, decay=LAMBDAS)
    ts = frontend.TracerSet(T.ROWS, T.COLS, T.DX, TT.functions(precision), initial=M0, decay=LAMBDAS)
    for s in (0, 3, 7):
        src = TT.SOURCE if s != 3 else TS.SOURCE_2
        dom.tracer_add_source(src["cells"], src["series"], species=s)
        ts.add_source(s, src["cells"], src["series"])
    assert dom.tracer_set_info() == dict(species=8, decay=list(LAMBDAS))
    sc = dom.read_scalars()
    dom.set_target_time(sc["time"] + 5.5 * sc["timestep"])
    suspended = 0
    for k in range(9):
        state, sc = dom.download(), dom.read_scalars()
        dom.step_batch(1)
        ts.apply(state, bed, sc["timestep"], sc["time"])
        suspended += not sc["timestep"] > 0
        got = read_all(dom, 8)
        for s in range(8):
            assert np.array_equal(got[s], ts.M[s]), (k, s) + differing(got[s], ts.M[s])
    totals = ts.branch_totals()
    print(totals, suspended)
    assert suspended > 0 and all(totals[name] > 0 for name in frontend.Tracer.BRANCHES + ("decayed",)), totals
    assert ts[0].branch_totals()["decayed"] == 0 and ts[6].branch_totals()["decayed"] > 0
    dom.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("cols,rows", [(5, 5), (67, 9), (130, 6), (66, 7), (64, 3), (3, 40)], ids=["5x5", "67x9", "130x6", "66x7", "64x3", "3x40"])
def test_tile_and_wave_edges(cols, rows, precision):
    """A partial wave, 64 + 3 columns, three waves a row, 64 + 2 (a block of halo columns only), rows that are no multiple of the
    block's four, a tile whose halo rows are the ring: a tilted wet surface over a rough bed, random M >= 0, one iteration, two
    species of which the second decays.  Ring cells come back copied, then decayed."""
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
    M0 = rng.random((2, rows, cols)) * (rng.random((2, rows, cols)) > 0.2)
    M0[:, 0, 0] = M0[:, -1, -1] = 0.75                                         # (ring cells that certainly hold something)
    dom = hp.Domain(cols, rows, dx=1.0, precision=precision, math_mode=hp.MATH_STRICT)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.tracer_enable_set(initial=M0, decay=(0.0, 0.5))
    sc = dom.read_scalars()
    dom.step_batch(1)
    ts = frontend.TracerSet(rows, cols, 1.0, TT.functions(precision, dx=1.0), initial=M0, decay=(0.0, 0.5))
    assert ts.apply(st, bed, sc["timestep"], sc["time"]) == (cols - 2) * (rows - 2)
    got = read_all(dom, 2)
    for s in range(2):
        assert np.array_equal(got[s], ts.M[s]), (s,) + differing(got[s], ts.M[s])
    ring = np.ones((rows, cols), bool)
    ring[1:-1, 1:-1] = False
    dt = np.float64(real(sc["timestep"]))
    assert dt > 0 and np.array_equal(got[0][ring], M0[0][ring]) and np.array_equal(got[1][ring], M0[1][ring] / (1.0 + 0.5 * dt))
    assert (got[1][ring] < M0[1][ring]).any() and not np.array_equal(got[0][~ring], M0[0][~ring])
    # the single tracer's kernel on the same water: species 0 in every bit
    single = hp.Domain(cols, rows, dx=1.0, precision=precision, math_mode=hp.MATH_STRICT)
    single.upload(st, bed, man)
    single.set_target_time(1e9)
    single.tracer_enable(M0[0])
    single.step_batch(1)
    assert np.array_equal(single.tracer_read(), got[0])
    single.close()
    dom.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_decay_alone_on_still_water():
    """Level water over a level bed, no boundary: M does not move.  Species 1 is the running M / (1 + lambda * dt_i) with the
    timestep read before each iteration, species 0 never changes a bit; at the target time the iterations are suspended (dt <= 0)
    and decay nothing."""
    cols, rows = 12, 9
    st = np.zeros((rows, cols, 4))
    st[..., 0] = st[..., 1] = 1.5
    bed, man = np.zeros((rows, cols)), np.full((rows, cols), 0.03)
    bed[4, 5] = st[4, 5, 0] = st[4, 5, 1] = 2.0                                # a dry pedestal: residue on dry ground decays too
    M0 = np.random.default_rng(4).random((2, rows, cols)) + 0.25
    dom = hp.Domain(cols, rows, dx=2.0, math_mode=hp.MATH_FAST)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.tracer_enable_set(initial=M0, decay=(0.0, 2.0))
    running = M0[1].copy()
    for k in range(10):
        dt = dom.read_scalars()["timestep"]
        dom.step_batch(1)
        assert dt > 0
        running = running / (1.0 + 2.0 * dt)
        assert np.array_equal(dom.tracer_read(species=1), running), k
        assert np.array_equal(dom.tracer_read(species=0), M0[0]), k
    assert (running < 0.9 * M0[1]).all()
    sc = dom.read_scalars()
    dom.set_target_time(sc["time"] + 1.5 * sc["timestep"])
    suspended = 0
    for k in range(5):
        dt = dom.read_scalars()["timestep"]
        dom.step_batch(1)
        if dt > 0:
            running = running / (1.0 + 2.0 * dt)
        else:
            suspended += 1
        assert np.array_equal(dom.tracer_read(species=1), running) and np.array_equal(dom.tracer_read(species=0), M0[0]), k
    assert suspended > 0
    dom.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
def enable_three(dom, decay=(0.0, 0.5, 0.0)):
    dom.tracer_enable_set(initial=TS.planes(), decay=decay)
    dom.tracer_add_source(TT.SOURCE["cells"], TT.SOURCE["series"])
    dom.tracer_add_source(TS.SOURCE_2["cells"], TS.SOURCE_2["series"], species=2)


@pytest.mark.parametrize("math_mode", [hp.MATH_FAST, hp.MATH_STRICT], ids=["fast", "strict"])
def test_save_and_restore_carry_every_plane(math_mode):
    dom = make(math_mode)[0]
    add_rain(dom)
    add_inflow(dom)
    enable_three(dom)
    dom.step_batch(5)                                     # an odd number: the checkpoint's planes lie in the second buffer
    dom.state_save()
    at_save = read_all(dom, 3)
    dom.step_batch(10)
    device = lambda sc: {k: v for k, v in sc.items() if k not in ("cells_calculated", "iterations")}      # (the host's own counts run on)
    first = (dom.download(), device(dom.read_scalars()), read_all(dom, 3))
    assert not np.array_equal(first[2], at_save) and dom.tracer_info()["iterations"] == 15
    dom.state_restore()
    assert np.array_equal(read_all(dom, 3), at_save) and dom.tracer_info()["iterations"] == 5
    dom.step_batch(10)
    again = (dom.download(), device(dom.read_scalars()), read_all(dom, 3))
    assert np.array_equal(first[0], again[0]) and first[1] == again[1] and np.array_equal(first[2], again[2])
    dom.close()


@pytest.mark.parametrize("before", ["nothing", "single", "set_of_two"])
def test_a_save_of_another_tracer_is_stale(before):
    """A checkpoint taken without a tracer, with a single tracer or with a set of another K, restored on a set of three: one
    warning, every plane left alone -- and the copy, sized for what was saved, is not read past its end."""
    dom = make(hp.MATH_FAST)[0]
    add_inflow(dom)
    if before == "single":
        dom.tracer_enable(TT.blob())
    elif before == "set_of_two":
        dom.tracer_enable_set(species=2)
    dom.step_batch(3)
    dom.state_save()
    dom.tracer_disable()
    lines = []
    hp.set_log_sink(lambda level, text: lines.append((level, text)))
    try:
        enable_three(dom)
        dom.step_batch(4)
        moved = read_all(dom, 3)
        dom.state_restore()
        M = read_all(dom, 3)
    finally:
        hp.set_log_sink(None)
    assert np.array_equal(M, moved) and not np.array_equal(moved, TS.planes()) and dom.tracer_info()["iterations"] == 4
    warnings = [text for level, text in lines if level == 8]
    assert len(warnings) == 1 and "tracer was enabled or disabled" in warnings[0], lines
    dom.step_batch(3)
    dom.state_save()                                      # ... and the next save holds all three planes
    kept = read_all(dom, 3)
    dom.step_batch(2)
    dom.state_restore()
    assert np.array_equal(read_all(dom, 3), kept) and np.isfinite(dom.download()).all()
    dom.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_the_single_tracer_calls_act_on_species_zero():
    dom = make(hp.MATH_FAST)[0]
    M0 = TS.planes()
    dom.tracer_enable_set(initial=M0, decay=(0.0, 0.25, 3.0))
    assert np.array_equal(dom.tracer_read(), M0[0]) and np.array_equal(read_all(dom, 3), M0)
    rows = np.random.default_rng(5).random((7, T.COLS))
    dom.tracer_write(rows, row0=11)                        # species 0
    dom.tracer_write(2.0 * rows, row0=3, species=2)
    want = M0.copy()
    want[0, 11:18] = rows
    want[2, 3:10] = 2.0 * rows
    assert np.array_equal(read_all(dom, 3), want) and np.array_equal(dom.tracer_read(row0=3, nrows=7, species=2), 2.0 * rows)
    dom.tracer_add_source(TT.SOURCE["cells"], TT.SOURCE["series"])                       # species 0
    dom.tracer_add_source(TT.SOURCE["cells"], TT.SOURCE["series"], species=1)            # the same cells, another species
    with pytest.raises(hp.HipimsError, match="listed twice"):                            # ... but (9, 8) is species 1's already
        dom.tracer_add_source(TS.SOURCE_2["cells"], TS.SOURCE_2["series"], species=1)
    assert dom.tracer_info() == dict(iterations=0, sources=2, source_cells=6)
    dom.close()


def test_what_was_written_and_fed_is_what_moves():
    dom = make(hp.MATH_FAST)[0]
    M0, decay = TS.planes(), (0.0, 0.25, 3.0)
    dom.tracer_enable_set(initial=M0, decay=decay)
    dom.tracer_write(np.full((2, T.COLS), 0.5), row0=8, species=1)
    M0[1, 8:10] = 0.5
    ts = frontend.TracerSet(T.ROWS, T.COLS, T.DX, TT.functions("f64"), initial=M0, decay=decay)
    for s, src in ((0, TT.SOURCE), (1, TT.SOURCE), (2, TS.SOURCE_2)):
        dom.tracer_add_source(src["cells"], src["series"], species=s)
        ts.add_source(s, src["cells"], src["series"])
    assert dom.tracer_info() == dict(iterations=0, sources=3, source_cells=8)
    bed = dom.download(hp.ARRAY_BED)
    for k in range(3):
        state, sc = dom.download(), dom.read_scalars()
        dom.step_batch(1)
        ts.apply(state, bed, sc["timestep"], sc["time"])
        assert np.array_equal(read_all(dom, 3), ts.M), k
    dom.tracer_sources_clear()                             # all of them
    assert dom.tracer_info() == dict(iterations=3, sources=0, source_cells=0)
    dom.tracer_add_source(TT.SOURCE["cells"], TT.SOURCE["series"], species=2)
    dom.tracer_disable()
    assert dom.tracer_set_info() == dict(species=0, decay=[]) and dom.tracer_info() == dict(iterations=0, sources=0, source_cells=0)
    dom.tracer_disable()                                  # idempotent
    dom.tracer_enable(TT.blob())                          # a single tracer is a set of one to the per-species calls
    assert dom.tracer_set_info() == dict(species=1, decay=[0.0])
    raster = np.zeros((1, T.COLS))
    assert dom.lib.hp_tracer_read_species(dom.h, 0, raster.ctypes.data, 14, 1) == 0
    dom.sync()
    assert np.array_equal(raster[0], TT.blob()[14]) and dom.lib.hp_tracer_read_species(dom.h, 1, raster.ctypes.data, 14, 1) == INVALID
    dom.close()


def test_refusals_and_argument_errors():
    last = lambda dom: dom.lib.hp_last_error().decode()
    # what hp_tracer_enable refuses, for the same reasons
    for scheme in (hp.SCHEME_MUSCL_HANCOCK, hp.SCHEME_INERTIAL):
        dom = make(hp.MATH_FAST, scheme=scheme)[0]
        assert raw_enable_set(dom, 2) == UNSUPPORTED and "Godunov" in last(dom)
        assert dom.tracer_set_info()["species"] == 0
        dom.step_batch(2)
        dom.close()
    st, bed, man, links = T.scene()
    g = strips.ghost_rows(hp.SCHEME_GODUNOV)
    own_lo, own_hi, lo, hi = strips.partition(T.ROWS, 2, g)[0]
    dom = hp.Domain(T.COLS, hi - lo, dx=T.DX, global_rows=T.ROWS, row_offset=lo, ghost_rows=g)
    dom.upload(st[lo:hi], bed[lo:hi], man[lo:hi])
    assert raw_enable_set(dom, 2) == UNSUPPORTED and "strip" in last(dom)
    dom.close()
    soil = TI.soil_scene()[3]
    packed = hp.pack_links(links, T.COLS)
    dom = make()[0]
    dom.add_links(links)
    assert raw_enable_set(dom, 2) == UNSUPPORTED and "link" in last(dom)
    dom.close()
    dom = make()[0]
    dom.add_infiltration(soil, TI.CLASSES)
    assert raw_enable_set(dom, 2) == UNSUPPORTED and "infiltration" in last(dom)
    dom.close()
    # ... and the reverse orders; a second enable of either form
    dom = make()[0]
    assert raw_enable_set(dom, 3, decay=(0.0, 1.0, 2.0), initial=TS.planes()) == 0
    assert dom.lib.hp_boundary_add_links(dom.h, packed.ctypes.data, len(packed)) == UNSUPPORTED and "tracer" in last(dom)
    assert raw_add(dom, soil) == UNSUPPORTED and "tracer" in last(dom)
    assert dom.links_info()["links"] == 0 and dom.infiltration_info() == dict(classes=0, pervious_cells=0)
    assert raw_enable_set(dom, 2) == STATE and "already" in last(dom)
    desc = hp.TracerDesc(C.sizeof(hp.TracerDesc), 0, None)
    assert dom.lib.hp_tracer_enable(dom.h, C.byref(desc)) == STATE and "already" in last(dom)
    single = make()[0]
    single.tracer_enable()
    assert raw_enable_set(single, 2) == STATE and "already" in last(single)
    single.close()
    # argument errors, before any device call
    assert raw_enable_set(dom, 0) == INVALID and "species outside 1..8" in last(dom)
    assert raw_enable_set(dom, 9) == INVALID and "species outside 1..8" in last(dom)
    assert raw_enable_set(dom, 2, struct_size=16) == INVALID and dom.lib.hp_tracer_enable_set(dom.h, None) == INVALID
    assert raw_enable_set(dom, 2, decay=(0.0, -1.0)) == INVALID and "species 1: the decay rate" in last(dom)
    assert raw_enable_set(dom, 2, decay=(np.nan, 1.0)) == INVALID and "species 0: the decay rate" in last(dom)
    bad = TS.planes()
    bad[2, 2, 5] = -1.0
    assert raw_enable_set(dom, 3, initial=bad) == INVALID and f"species 2, cell {2 * T.COLS + 5}:" in last(dom)
    cells, series = np.array([9 * T.COLS + 9], np.uint64), np.array([(0.0, 1.0)])
    add = lambda s, c, ser: dom.lib.hp_tracer_add_source_to(dom.h, s, c.ctypes.data, len(c), ser.ctypes.data, len(ser))
    assert add(3, cells, series) == INVALID and "species 3 of a tracer of 3" in last(dom)
    assert add(1, np.array([5], np.uint64), series) == INVALID and "edge ring" in last(dom)
    assert add(1, cells, series) == 0 and add(1, cells, series) == INVALID and "listed twice" in last(dom)
    assert add(2, cells, series) == 0 and dom.lib.hp_tracer_add_source(dom.h, cells.ctypes.data, 1, series.ctypes.data, 1) == 0
    assert dom.tracer_info() == dict(iterations=0, sources=3, source_cells=3)
    raster = np.zeros((T.ROWS + 1, T.COLS))
    assert dom.lib.hp_tracer_read_species(dom.h, 3, raster.ctypes.data, 0, 1) == INVALID and "species 3" in last(dom)
    assert dom.lib.hp_tracer_write_species(dom.h, 8, raster.ctypes.data, 0, 1) == INVALID
    assert dom.lib.hp_tracer_read_species(dom.h, 2, None, 0, 1) == INVALID and dom.lib.hp_tracer_write_species(dom.h, 2, None, 0, 1) == INVALID
    for row0, nrows in ((0, T.ROWS + 1), (-1, 2), (T.ROWS, 1), (3, -1)):
        assert dom.lib.hp_tracer_read_species(dom.h, 2, raster.ctypes.data, row0, nrows) == INVALID, (row0, nrows)
        assert dom.lib.hp_tracer_write_species(dom.h, 2, raster.ctypes.data, row0, nrows) == INVALID, (row0, nrows)
    # between hp_step_begin and hp_step_end
    dom.step_begin()
    assert dom.lib.hp_tracer_read_species(dom.h, 2, raster.ctypes.data, 0, 1) == STATE
    assert dom.lib.hp_tracer_write_species(dom.h, 2, raster.ctypes.data, 0, 1) == STATE
    assert add(0, np.array([10 * T.COLS + 10], np.uint64), series) == STATE and raw_enable_set(dom, 2) == STATE
    dom.step_end()
    dom.step_batch(2)
    dom.tracer_disable()
    assert dom.lib.hp_tracer_read_species(dom.h, 0, raster.ctypes.data, 0, 1) == STATE and add(0, cells, series) == STATE
    dom.tracer_disable()                                  # idempotent
    dom.step_batch(2)
    dom.close()


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_model_writes_every_species(tmp_path):
    from hipims_mi.model import Model
    xml, m0 = TS.write_model(tmp_path)
    m = Model(xml, output_format=".npy")
    assert m.sim.tracer_set_info() == dict(species=2, decay=[0.0, 0.25]) and m.sim.tracer_info() == dict(iterations=0, sources=2, source_cells=4)
    m.run()
    out = tmp_path / "out"
    river, sewage = m.sim.tracer_read(species=0), m.sim.tracer_read(species=1)
    assert np.array_equal(np.load(out / "tracer_river_2.npy"), river) and np.array_equal(np.load(out / "tracer_sewage_2.npy"), sewage)
    assert np.array_equal(np.load(out / "conc_river_2.npy"), frontend.tracer_concentration(river, m.sim.download(), m.bed))
    assert np.array_equal(np.load(out / "sewage_conc_2.npy"), frontend.tracer_concentration(sewage, m.sim.download(), m.bed))
    assert river[3, 3] > 0 and sewage[20, 30] > 0 and sewage[3, 3] == 0 and m0[3, 3] == 0 and m.sim.tracer_info()["iterations"] > 0
    m.sim.close()
