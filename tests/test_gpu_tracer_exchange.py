"""A tracer species' exchange with the bed on the GPU (hp_tracer_set_exchange; csrc/hp_tracer.hpp: tracer_step_set<T, true>,
tracer_exchange).  The reference is frontend.TracerSet(exchange=...), the NumPy restatement with step 7, and the same set without the
call.  Every comparison is array_equal; everything runs at 40 x 32 cells or smaller, but for the 130- and 67-column shapes of the
wave-edge cases."""
import ctypes as C

import numpy as np
import pytest

import hipims_mi as hp
import test_links as T
import test_tracer as TT
import test_tracer_exchange as TX
import test_tracer_set as TS
from hipims_mi import frontend
from test_gpu_tracer import INVALID, REAL, STATE, UNSUPPORTED, add_inflow, add_rain, differing, make
from test_gpu_tracer_set import read_all

pytestmark = pytest.mark.gpu
INF = float("inf")
# the scene's bed shear stress lies in [0, 1.4e-3] N/m2 once the inflow has set the water in motion (most of it below 1e-7, sixteen cells
# above 1e-5: measured on the restatement): species 1's thresholds lie inside that range
EXCHANGE = [dict(settling=2e-2),                                                                  # a pure depositor: tau_deposit = +inf
            dict(settling=1e-2, tau_deposit=1e-6, tau_erode=1e-5, erodibility=5e-3),              # Krone and Partheniades
            dict(settling=5e-3, tau_deposit=1e-6, tau_erode=2e-5, erodibility=1e-3),              # ... with a decay
            None]                                                                                 # no exchange
DECAY = (0.0, 0.0, 0.5, 0.25)


def deposits():
    """D0 of the four species: zeros, a layer everywhere, a patch, zeros."""
    y, x = np.mgrid[0:T.ROWS, 0:T.COLS].astype(np.float64)
    return np.stack([np.zeros((T.ROWS, T.COLS)), 0.125 + x / 256.0 + y / 512.0, np.where((x > 4) & (x < 18), 0.25, 0.0), np.zeros((T.ROWS, T.COLS))])


def initial():
    rng = np.random.default_rng(9)
    return np.stack([TT.blob() * (s + 1) + (rng.random((T.ROWS, T.COLS)) < 0.3) * rng.random((T.ROWS, T.COLS)) for s in range(4)])


def set_exchange(dom, exchange, deposit=None):
    for s, q in enumerate(exchange):
        if q is not None:
            dom.tracer_set_exchange(s, deposit=None if deposit is None else deposit[s], **q)


def read_deposits(dom, species):
    return np.stack([dom.tracer_deposit_read(species=s) for s in range(species)])


def raw_set_exchange(dom, species, settling=0.0, tau_deposit=INF, tau_erode=INF, erodibility=0.0, deposit=None, struct_size=None):
    """hp_tracer_set_exchange itself: the return code."""
    d0 = None if deposit is None else np.ascontiguousarray(deposit, np.float64)
    desc = hp.TracerExchangeDesc(C.sizeof(hp.TracerExchangeDesc) if struct_size is None else struct_size, species, settling, tau_deposit, tau_erode,
                                 erodibility, None if d0 is None else d0.ctypes.data)
    return dom.lib.hp_tracer_set_exchange(dom.h, C.byref(desc))


def run_against_the_restatement(dom, bed, man, precision, iterations=9):
    """Four species on `dom` (its water in motion, no boundary left), batches of one iteration across a target time: after every
    iteration every plane of M and D equals frontend.TracerSet.apply on the state and the timestep the iteration started from."""
    M0, D0 = initial(), deposits()
    dom.tracer_enable_set(initial=M0, decay=DECAY)
    set_exchange(dom, EXCHANGE, D0)
    ts = frontend.TracerSet(T.ROWS, T.COLS, T.DX, TT.functions(precision), initial=M0, decay=DECAY, exchange=EXCHANGE, deposit=D0, manning=man)
    for s in (0, 3):
        dom.tracer_add_source(TT.SOURCE["cells"], TT.SOURCE["series"], species=s)
        ts.add_source(s, TT.SOURCE["cells"], TT.SOURCE["series"])
    assert dom.tracer_exchange_info()["exchanging"] == 3 and np.array_equal(read_deposits(dom, 4), D0)
    sc = dom.read_scalars()
    dom.set_target_time(sc["time"] + 5.5 * sc["timestep"])
    suspended = 0
    for k in range(iterations):
        state, sc = dom.download(), dom.read_scalars()
        dom.step_batch(1)
        ts.apply(state, bed, sc["timestep"], sc["time"])
        suspended += not sc["timestep"] > 0
        M, D = read_all(dom, 4), read_deposits(dom, 4)
        for s in range(4):
            assert np.array_equal(M[s], ts.M[s]), ("M", k, s) + differing(M[s], ts.M[s])
            assert np.array_equal(D[s], ts.D[s]), ("D", k, s) + differing(D[s], ts.D[s])
    totals = ts.branch_totals()
    print(totals, suspended, [t.branch_totals()["eroded"] for t in ts.tracers])
    assert suspended > 0 and totals["deposited"] > 0 and totals["eroded"] > 0 and totals["moved"] > 0 and totals["decayed"] > 0, totals
    assert ts[1].branch_totals()["deposited"] > 0 and ts[1].branch_totals()["eroded"] > 0 and ts[2].branch_totals()["deposited"] > 0
    assert ts[0].branch_totals()["eroded"] == 0 == ts[3].branch_totals()["deposited"] and not ts.D[3].any() and not np.array_equal(ts.D[:3], D0[:3])


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_four_species_equal_the_restatement(precision):
    """STRICT: the scene and the inflow of test_eight_decaying_species_equal_the_restatement (the inflow sets the water in motion and
    is then cleared: the restatement is handed the downloaded state)."""
    real = REAL[precision]
    st, bed, man = (a.astype(real) for a in TT.traced_scene())
    dom = hp.Domain(T.COLS, T.ROWS, dx=T.DX, precision=precision, math_mode=hp.MATH_STRICT)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    add_inflow(dom)
    dom.step_batch(6)
    dom.clear_boundaries()
    run_against_the_restatement(dom, bed, man, precision)
    dom.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_fast_iterations_exchange_by_the_same_arithmetic():
    """FAST math: the water differs from STRICT's, the tracer's arithmetic on it does not."""
    st, bed, man = TT.traced_scene()
    dom = hp.Domain(T.COLS, T.ROWS, dx=T.DX, math_mode=hp.MATH_FAST)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    add_inflow(dom)
    dom.step_batch(6)
    dom.clear_boundaries()
    run_against_the_restatement(dom, bed, man, "f64")
    assert dom.pair_stats()["pairs"] == 0
    dom.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [False, True], ids=["manning_array", "manning_uniform"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("cols,rows", [(5, 5), (67, 9), (130, 6), (66, 7), (64, 3), (3, 40)], ids=["5x5", "67x9", "130x6", "66x7", "64x3", "3x40"])
def test_tile_and_wave_edges(cols, rows, precision, uniform):
    """The shapes of the set's test_tile_and_wave_edges: a tilted wet surface over a rough bed, one iteration, two species of which the
    second exchanges (its thresholds inside the water's shear stress, 0.01 to 0.5 N/m2), a Manning array and a uniform value.  Ring
    cells and a disabled cell keep M'' and D."""
    rng = np.random.default_rng(cols * 100 + rows)
    real = REAL[precision]
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    bed = np.round(0.2 * rng.random((rows, cols)), 4)
    st = np.zeros((rows, cols, 4))
    st[..., 0] = 1.0 + 0.004 * x - 0.01 * y
    st[..., 2] = np.round(0.1 * rng.standard_normal((rows, cols)), 4)
    st[..., 3] = np.round(0.1 * rng.standard_normal((rows, cols)), 4)
    st[..., 1] = st[..., 0]
    man = np.full((rows, cols), 0.03) if uniform else np.round(0.02 + 0.03 * rng.random((rows, cols)), 4)
    off = (rows // 2, cols // 2)                                               # one disabled cell inside the ring
    st[off][1] = -9999.0
    st, bed, man = st.astype(real), bed.astype(real), man.astype(real)
    M0 = rng.random((2, rows, cols)) * (rng.random((2, rows, cols)) > 0.2)
    D0 = np.stack([np.zeros((rows, cols)), 0.5 * rng.random((rows, cols)) * (rng.random((rows, cols)) > 0.3)])
    M0[:, 0, 0] = M0[:, -1, -1] = D0[1, 0, 0] = D0[1, -1, -1] = 0.75           # (ring cells that certainly hold something)
    M0[(slice(None),) + off], D0[(1,) + off] = 0.5, 0.375
    q = dict(settling=1e-2, tau_deposit=0.08, tau_erode=0.12, erodibility=2e-2)
    dom = hp.Domain(cols, rows, dx=1.0, precision=precision, math_mode=hp.MATH_STRICT)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.tracer_enable_set(initial=M0, decay=(0.0, 0.5))
    dom.tracer_set_exchange(1, deposit=D0[1], **q)
    sc = dom.read_scalars()
    dom.step_batch(1)
    ts = frontend.TracerSet(rows, cols, 1.0, TT.functions(precision, dx=1.0), initial=M0, decay=(0.0, 0.5), exchange=[None, q], deposit=D0, manning=man)
    assert ts.apply(st, bed, sc["timestep"], sc["time"]) == (cols - 2) * (rows - 2) - 1
    M, D = read_all(dom, 2), read_deposits(dom, 2)
    for s in range(2):
        assert np.array_equal(M[s], ts.M[s]), ("M", s) + differing(M[s], ts.M[s])
        assert np.array_equal(D[s], ts.D[s]), ("D", s) + differing(D[s], ts.D[s])
    kept = np.ones((rows, cols), bool)
    kept[1:-1, 1:-1] = False
    kept[off] = True
    dt = np.float64(real(sc["timestep"]))
    assert dt > 0 and np.array_equal(D[1][kept], D0[1][kept]) and np.array_equal(M[1][kept], M0[1][kept] / (1.0 + 0.5 * dt)) and not D[0].any()
    totals = ts[1].branch_totals()
    if cols * rows > 25:
        assert totals["deposited"] > 0 and totals["eroded"] > 0, totals
    assert totals["deposited"] + totals["eroded"] > 0 and not np.array_equal(D[1], D0[1])
    # the same set without the call: species 0 in every bit
    plain = hp.Domain(cols, rows, dx=1.0, precision=precision, math_mode=hp.MATH_STRICT)
    plain.upload(st, bed, man)
    plain.set_target_time(1e9)
    plain.tracer_enable_set(initial=M0, decay=(0.0, 0.5))
    plain.step_batch(1)
    assert np.array_equal(plain.tracer_read(species=0), M[0]) and not np.array_equal(plain.tracer_read(species=1), M[1])
    plain.close()
    dom.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_a_block_without_a_moving_cell_beside_blocks_that_move():
    """40 x 32, rows 16 and above dry, level ground: the blocks of rows 20 to 31 have no moving cell and take the kernel's early path,
    the blocks below exchange, all in one launch.  D on the dry side is untouched in every bit, M there only decays."""
    cols, rows = T.COLS, T.ROWS
    rng = np.random.default_rng(44)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    bed = np.where(y >= 16, 3.0, np.round(0.1 * rng.random((rows, cols)), 4))
    st = np.zeros((rows, cols, 4))
    st[..., 0] = np.maximum(bed, 1.0 + 0.005 * x)
    st[..., 1] = st[..., 0]
    st[:16, :, 2] = np.round(0.2 * rng.standard_normal((16, cols)), 4)
    man = np.full((rows, cols), 0.03)
    M0 = rng.random((2, rows, cols)) + 0.25
    D0 = rng.random((2, rows, cols)) + 0.125
    q = [dict(settling=1e-2, tau_deposit=0.1, tau_erode=0.2, erodibility=1e-2), dict(settling=3e-2, erodibility=0.0)]
    dom = hp.Domain(cols, rows, dx=2.0, math_mode=hp.MATH_STRICT)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.tracer_enable_set(initial=M0, decay=(0.0, 0.5))
    set_exchange(dom, q, D0)
    ts = frontend.TracerSet(rows, cols, 2.0, TT.functions("f64", dx=2.0), initial=M0, decay=(0.0, 0.5), exchange=q, deposit=D0, manning=man)
    for k in range(3):
        state, sc = dom.download(), dom.read_scalars()
        dom.step_batch(1)
        ts.apply(state, bed, sc["timestep"], sc["time"])
        M, D = read_all(dom, 2), read_deposits(dom, 2)
        assert np.array_equal(M, ts.M) and np.array_equal(D, ts.D), (k,) + differing(D, ts.D)
        assert np.array_equal(D[:, 17:], D0[:, 17:]) and np.array_equal(M[0, 17:], M0[0, 17:]) and (M[1, 17:] < M0[1, 17:]).all()
    assert ts[0].branches["moved"][20:].sum() == 0 and ts[0].branches["moved"][:15].sum() > 0
    assert ts[0].branch_totals()["deposited"] > 0 and ts[0].branch_totals()["eroded"] > 0 and not np.array_equal(D[:, :15], D0[:, :15])
    dom.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math_mode", [hp.MATH_FAST, hp.MATH_STRICT], ids=["fast", "strict"])
def test_zero_parameters_are_no_exchange(math_mode):
    """hp_tracer_set_exchange with settling = 0 and erodibility = 0 on every species: water, scalars, every plane of M, launch counts
    and pair statistics are those of the set without the call.  Then one species with exchange: the water and the OTHER species' M
    are still those."""
    M0, decay = TS.planes(), (0.0, 0.5, 0.0)

    def run(exchange):
        dom = make(math_mode)[0]
        dom.tracer_enable_set(initial=M0, decay=decay)
        dom.tracer_add_source(TT.SOURCE["cells"], TT.SOURCE["series"])
        dom.tracer_add_source(TS.SOURCE_2["cells"], TS.SOURCE_2["series"], species=2)
        add_rain(dom)
        add_inflow(dom)
        set_exchange(dom, exchange, deposits()[:3])
        out = []
        for n in (1, 3, 7, 4):
            dom.step_batch(n)
            out.append((dom.download(), dom.read_scalars(), read_all(dom, 3)))
        pairs = {k: v for k, v in dom.pair_stats().items() if k != "pair_over_single"}      # (all counts but that one, a measured ratio)
        counts, info = dom.launch_counts(), dom.tracer_exchange_info()
        D = read_deposits(dom, 3) if info["exchanging"] else None
        dom.close()
        return out, counts, pairs, info, D

    plain = run([None, None, None])
    zeros = run([dict(settling=0.0, tau_deposit=0.5, tau_erode=1.0, erodibility=0.0)] * 3)
    assert plain[3]["exchanging"] == 0 == zeros[3]["exchanging"] and zeros[3]["species"][1]["tau_erode"] == 1.0
    assert zeros[1] == plain[1] and zeros[2] == plain[2]
    for a, b in zip(plain[0], zeros[0]):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    one = run([None, dict(settling=2e-2, tau_deposit=1e-6, tau_erode=1e-5, erodibility=5e-3), None])
    assert one[3]["exchanging"] == 1 and one[1] == plain[1] and one[2] == plain[2]
    for a, b in zip(plain[0], one[0]):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][2], b[2][2])
    assert not np.array_equal(plain[0][-1][2][1], one[0][-1][2][1]) and not np.array_equal(one[4][1], deposits()[1])
    assert not one[4][0].any() and not one[4][2].any()                        # the planes of the others stay zero: never touched


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_deposit():
    dom = make(hp.MATH_FAST)[0]
    add_rain(dom)
    add_inflow(dom)
    dom.tracer_enable_set(initial=initial(), decay=DECAY)
    dom.step_batch(2)
    dom.state_save()                                      # before the first hp_tracer_set_exchange: stale afterwards
    set_exchange(dom, EXCHANGE, deposits())
    dom.step_batch(3)
    lines = []
    hp.set_log_sink(lambda level, text: lines.append((level, text)))
    try:
        moved = (read_all(dom, 4), read_deposits(dom, 4))
        dom.state_restore()
        left = (read_all(dom, 4), read_deposits(dom, 4))
    finally:
        hp.set_log_sink(None)
    assert np.array_equal(left[0], moved[0]) and np.array_equal(left[1], moved[1]) and not np.array_equal(moved[1], deposits())
    warnings = [text for level, text in lines if level == 8]
    assert len(warnings) == 1 and "tracer" in warnings[0] and "exchange" in warnings[0], lines
    assert dom.tracer_info()["iterations"] == 5
    # save, three iterations, restore, three iterations: M and D repeat in every bit
    dom.state_save()
    at_save = (read_all(dom, 4), read_deposits(dom, 4))
    dom.step_batch(3)
    first = (dom.download(), read_all(dom, 4), read_deposits(dom, 4))
    assert not np.array_equal(first[2], at_save[1]) and not np.array_equal(first[1], at_save[0])
    dom.state_restore()
    assert np.array_equal(read_all(dom, 4), at_save[0]) and np.array_equal(read_deposits(dom, 4), at_save[1]) and dom.tracer_info()["iterations"] == 5
    dom.step_batch(3)
    again = (dom.download(), read_all(dom, 4), read_deposits(dom, 4))
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    # a second hp_tracer_set_exchange (new parameters, deposit_initial = NULL) keeps D and does not stale the snapshot
    lines = []
    hp.set_log_sink(lambda level, text: lines.append((level, text)))
    try:
        dom.tracer_set_exchange(1, settling=4e-2, tau_deposit=1e-6, tau_erode=1e-5, erodibility=1e-3)
        dom.tracer_set_exchange(3, settling=1e-3)
        assert np.array_equal(read_deposits(dom, 4), again[2]) and dom.tracer_exchange_info()["exchanging"] == 4
        dom.state_restore()
    finally:
        hp.set_log_sink(None)
    assert not [text for level, text in lines if level == 8], lines
    assert np.array_equal(read_all(dom, 4), at_save[0]) and np.array_equal(read_deposits(dom, 4), at_save[1])
    dom.step_batch(3)
    assert not np.array_equal(read_deposits(dom, 4)[1], again[2][1]) and read_deposits(dom, 4)[3].any()      # the new parameters hold
    dom.close()


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_calls_and_refusals():
    last = lambda dom: dom.lib.hp_last_error().decode()
    dom = make()[0]
    raster = np.zeros((T.ROWS + 1, T.COLS))
    read = lambda s, row0=0, nrows=1: dom.lib.hp_tracer_deposit_read(dom.h, s, raster.ctypes.data, row0, nrows)
    write = lambda s, row0=0, nrows=1: dom.lib.hp_tracer_deposit_write(dom.h, s, raster.ctypes.data, row0, nrows)
    # before a tracer exists
    assert raw_set_exchange(dom, 0, settling=1e-3) == STATE and "no tracer" in last(dom)
    assert read(0) == STATE and write(0) == STATE and dom.tracer_exchange_info() == dict(exchanging=0, species=[])
    # on hp_tracer_enable's single tracer
    dom.tracer_enable(TT.blob())
    assert raw_set_exchange(dom, 0, settling=1e-3) == UNSUPPORTED and "set of one" in last(dom)
    assert read(0) == STATE and "no species" in last(dom)
    dom.step_batch(2)
    dom.tracer_disable()
    # a set: argument errors before any device call, in the header's order
    dom.tracer_enable_set(initial=TS.planes(), decay=(0.0, 0.5, 0.0))
    assert read(0) == STATE and "no species" in last(dom) and write(1) == STATE                   # no species exchanges yet
    assert dom.lib.hp_tracer_set_exchange(dom.h, None) == INVALID and "desc == NULL" in last(dom)
    assert raw_set_exchange(dom, 0, settling=1e-3, struct_size=40) == INVALID and "size mismatch" in last(dom)
    assert raw_set_exchange(dom, 3, settling=1e-3) == INVALID and "species 3 of a tracer of 3" in last(dom)
    assert raw_set_exchange(dom, 0, settling=-1.0) == INVALID and "settling" in last(dom)
    assert raw_set_exchange(dom, 0, tau_deposit=0.0) == INVALID and "tau_deposit" in last(dom)
    assert raw_set_exchange(dom, 0, tau_deposit=1.0, tau_erode=0.5) == INVALID and "tau_erode" in last(dom)
    assert raw_set_exchange(dom, 0, erodibility=np.nan) == INVALID and "erodibility" in last(dom)
    bad = np.zeros((T.ROWS, T.COLS))
    bad[2, 5] = -1.0
    assert raw_set_exchange(dom, 0, settling=1e-3, deposit=bad) == INVALID and f"cell {2 * T.COLS + 5}: deposit_initial" in last(dom)
    assert dom.tracer_exchange_info()["exchanging"] == 0 and read(0) == STATE
    # inside a split step
    dom.step_begin()
    assert raw_set_exchange(dom, 0, settling=1e-3) == STATE and "hp_step_begin" in last(dom)
    dom.step_end()
    # set, read back, write and read
    d0 = np.random.default_rng(7).random((T.ROWS, T.COLS))
    dom.tracer_set_exchange(1, settling=1e-3, tau_deposit=0.5, tau_erode=2.0, erodibility=1e-4, deposit=d0)
    info = dom.tracer_exchange_info()
    assert info["exchanging"] == 1 and info["species"][1] == dict(settling=1e-3, tau_deposit=0.5, tau_erode=2.0, erodibility=1e-4)
    assert info["species"][0] == info["species"][2] == dict(settling=0.0, tau_deposit=INF, tau_erode=INF, erodibility=0.0)
    assert np.array_equal(dom.tracer_deposit_read(species=1), d0) and not dom.tracer_deposit_read(species=0).any()
    rows = np.random.default_rng(8).random((7, T.COLS))
    dom.tracer_deposit_write(rows, species=2, row0=11)
    dom.tracer_deposit_write(2.0 * rows, species=1, row0=3)
    d0[3:10] = 2.0 * rows
    assert np.array_equal(dom.tracer_deposit_read(species=1), d0) and np.array_equal(dom.tracer_deposit_read(species=2, row0=11, nrows=7), rows)
    assert np.array_equal(dom.tracer_deposit_read(species=1, row0=3, nrows=7), 2.0 * rows) and np.array_equal(read_all(dom, 3), TS.planes())
    assert read(3) == INVALID and "species 3" in last(dom) and write(8) == INVALID
    assert dom.lib.hp_tracer_deposit_read(dom.h, 1, None, 0, 1) == INVALID and dom.lib.hp_tracer_deposit_write(dom.h, 1, None, 0, 1) == INVALID
    for row0, nrows in ((0, T.ROWS + 1), (-1, 2), (T.ROWS, 1), (3, -1)):
        assert read(1, row0, nrows) == INVALID and write(1, row0, nrows) == INVALID, (row0, nrows)
    dom.step_begin()
    assert read(1) == STATE and write(1) == STATE
    dom.step_end()
    dom.step_batch(2)
    # zero parameters again: no species exchanges, D is kept but not handed out
    dom.tracer_set_exchange(1)
    assert dom.tracer_exchange_info()["exchanging"] == 0 and read(1) == STATE
    dom.tracer_set_exchange(1, settling=1e-3)
    kept = dom.tracer_deposit_read(species=1)
    assert kept.any() and np.array_equal(dom.tracer_deposit_read(species=2, row0=11, nrows=7), rows)
    # hp_tracer_disable frees D: a fresh set starts without one
    dom.tracer_disable()
    assert dom.tracer_exchange_info() == dict(exchanging=0, species=[]) and read(0) == STATE
    dom.tracer_enable_set(species=2)
    assert dom.tracer_exchange_info()["exchanging"] == 0 and read(0) == STATE
    dom.tracer_set_exchange(0, settling=1e-3)
    assert not read_deposits(dom, 2).any()
    dom.step_batch(2)
    dom.close()


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_model_writes_the_deposit(tmp_path):
    from hipims_mi.model import Model
    xml, m0, d0 = TX.write_model(tmp_path)
    m = Model(xml, output_format=".npy")
    info = m.sim.tracer_exchange_info()
    assert info["exchanging"] == 1 and info["species"][0] == dict(settling=0.001, tau_deposit=0.08, tau_erode=0.25, erodibility=0.0002)
    assert np.array_equal(m.sim.tracer_deposit_read(species=0), d0)
    m.run()
    out = tmp_path / "out"
    D, M = m.sim.tracer_deposit_read(species=0), m.sim.tracer_read(species=0)
    assert np.array_equal(np.load(out / "deposit_silt_2.npy"), D) and np.array_equal(np.load(out / "tracer_silt_2.npy"), M)
    assert not np.array_equal(np.load(out / "deposit_silt_1.npy"), D) and not np.array_equal(np.load(out / "deposit_silt_1.npy"), d0)
    assert D[6, 7] > d0[6, 7] == 0 and M[6, 7] < m0[6, 7] and m.sim.tracer_info()["iterations"] > 0       # still water under the patch: it settles
    m.sim.close()
