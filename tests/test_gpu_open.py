"""The open boundary on the GPU (hp_boundary_add_open; csrc/hp_open.hpp: bdy_open).  The reference is the stepwise loop over the oracle's
grid functions with frontend.Open.apply on the source buffer where the engine launches bdy_open (tests/test_links.py: StepLoop;
tests/test_open.py: scene, reference); STRICT runs and the records are compared bit for bit, FAST fp64 at the project's FAST tolerance."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import hipims_mi as hp
import oracle
import test_links as T
import test_open as O
from hipims_mi import frontend, strips

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COLS, ROWS, DX = O.COLS, O.ROWS, O.DX
same_records = lambda got, want: got.tobytes() == want.tobytes()


def same_scalars(sc, sr):
    return (sc["time"] == sr["t"] and sc["timestep"] == sr["dt"] and sc["time_hydrological"] == sr["t_hydro"] and sc["batch_timesteps"] == sr["batch_dt"]
            and sc["batch_successful"] == sr["batch_ok"] and sc["batch_skipped"] == sr["batch_skipped"])


def make(math_mode=hp.MATH_STRICT, precision="f64", scheme=hp.SCHEME_GODUNOV, all_wet=False):
    st, bed, man = O.scene(np.float64 if precision == "f64" else np.float32, all_wet=all_wet)
    dom = hp.Domain(COLS, ROWS, dx=DX, scheme=scheme, precision=precision, math_mode=math_mode)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    return dom, st, bed, man


def add_all(dom):
    """The uniform rain in front of the open boundary."""
    dom.add_uniform(T.RAIN["definition"], T.RAIN["series"], T.RAIN["interval"], T.RAIN["length"])
    dom.add_open(O.SEGMENTS)


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_strict_trajectory_is_the_reference_in_every_bit():
    ref = O.reference()
    assert all(ref["totals"][b] >= 1 for b in O.REQUIRED), ref["totals"]
    dom = make(hp.MATH_STRICT)[0]
    add_all(dom)
    assert not dom.boundaries_fused() and dom.open_info() == dict(segments=2, cells=36)
    for k, n in enumerate(O.BATCHES):
        dom.step_batch(n)
        state, sc, rec = ref["after"][k]
        assert np.array_equal(dom.download(), state), f"state after batch {k}"
        assert same_scalars(dom.read_scalars(), sc), (k, dom.read_scalars(), sc)
        got = dom.open_read()
        assert same_records(got, rec), (k, got, rec)
    assert dom.pair_stats()["pairs"] == 0 and not dom.boundaries_fused()
    dom.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_fast_trajectory_is_within_the_fast_tolerance():
    ref = O.reference()
    bed = ref["start"][1]
    dom = make(hp.MATH_FAST)[0]
    add_all(dom)
    for k, n in enumerate(O.BATCHES):
        dom.step_batch(n)
        state, sc, rec = ref["after"][k]
        got = dom.download()
        wet = bed <= 9999.0
        rmse = float(np.sqrt(np.mean(((got[..., 0] - state[..., 0])[wet]) ** 2)))
        r = dom.open_read()
        print("batch", k, "depth RMSE", rmse, "largest record difference: q_last", float(np.abs(r["q_last"] - rec["q_last"]).max()),
              "volume", float(np.abs(r["volume"] - rec["volume"]).max()))
        assert rmse < 1e-9, (k, rmse)
    assert dom.pair_stats()["pairs"] == 0
    dom.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
def twin(cols, rows, st, bed, man, segments, math_mode, precision):
    """Domain A with the open boundary against domain B, a fresh upload of the state the restatement has patched: one iteration each.
    The flux kernel never writes the ring, and after one iteration the download reads the buffer it wrote: there A's listed ring cells
    still hold what was uploaded, while B's hold the patch in both buffers.  So the two are compared in every bit everywhere else --
    the interior is what shows that the flux launch read the imposed ring -- and the imposed values themselves are read after A's second
    iteration, when the download reads the buffer the first one imposed on.
    Returns (the patched state, A's state after two iterations, A's records after one, the restatement)."""
    kw = dict(dx=DX, precision=precision, math_mode=math_mode)
    a, b = hp.Domain(cols, rows, **kw), hp.Domain(cols, rows, **kw)
    for d in (a, b):
        d.upload(st, bed, man)
        d.set_target_time(1e9)
    a.add_open(segments)
    dt0 = a.read_scalars()["timestep"]
    R = frontend.Open(rows, cols, DX, oracle.OracleFunctions(precision, dx=DX), segments)
    patched = st.copy()
    R.apply(patched, bed, dt0)
    b.upload(state=patched)
    a.step_batch(1)
    b.step_batch(1)
    after_a, after_b = a.download(), b.download()
    listed = np.zeros((rows, cols), bool)
    listed.reshape(-1)[R.cells] = True
    assert np.array_equal(after_a[~listed], after_b[~listed]) and not np.array_equal(after_a[1:-1, 1:-1], st[1:-1, 1:-1])
    assert np.array_equal(after_a[listed], st[listed]) and np.array_equal(after_b[listed], patched[listed])
    assert a.read_scalars() == b.read_scalars()
    rec = a.open_read()
    assert same_records(rec, R.records()), (rec, R.records())
    a.step_batch(1)
    second = a.download()
    assert np.array_equal(second[listed], patched[listed])                     # what the first iteration imposed, in every bit
    a.close(); b.close()
    return patched, second, rec, R


@pytest.mark.parametrize("math_mode", [hp.MATH_FAST, hp.MATH_STRICT], ids=["fast", "strict"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_one_iteration_is_its_twin(precision, math_mode):
    """All wet, so that no cell is left untouched by the flux kernel."""
    st, bed, man = O.scene(np.float64 if precision == "f64" else np.float32, all_wet=True)
    patched, after, rec, R = twin(COLS, ROWS, st, bed, man, O.SEGMENTS, math_mode, precision)
    assert not np.array_equal(patched, st) and int((rec["active"] > 0).sum()) >= 20 and R.branch_totals()["inward_zeroed"] >= 1


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_launch_shape():
    """150 x 9 with the whole south and north edges open: 2 x 148 cells in one call, five blocks of 64 lanes with a partial last wave,
    the third block holding lanes of both segments.  All wet: every listed ring cell changes, nothing else of the ring does."""
    cols, rows = 150, 9
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    bed = O.syn.round4(0.2 * np.sin(x / 7.0) + 0.05 * y)
    st = np.zeros((rows, cols, 4))
    st[..., 0] = st[..., 1] = O.syn.round4(1.5 + 0.3 * np.cos(x / 11.0))
    st[..., 3] = O.syn.round4(0.2 * np.where(y < rows / 2, -1.0, 1.0))        # outward on both edges
    O.syn._walls(st, bed)
    bed[0, 1:-1], bed[-1, 1:-1] = bed[1, 1:-1] - 0.02, bed[-2, 1:-1] - 0.02   # the two edges opened: ring cells dry at a real bed
    st[0, 1:-1, :2], st[-1, 1:-1, :2] = bed[0, 1:-1, None], bed[-1, 1:-1, None]
    man = np.full((rows, cols), 0.03)
    patched, after, rec, R = twin(cols, rows, st, bed, man, ["south", "north"], hp.MATH_STRICT, "f64")
    assert len(rec) == 296 and list(R.cells) == list(range(1, 149)) + [8 * cols + c for c in range(1, 149)]
    ring_changed = (after != st).any(axis=-1)                                                # (after A's second iteration: the buffer the first imposed on)
    assert ring_changed[0, 1:-1].all() and ring_changed[-1, 1:-1].all()                      # every listed ring cell
    assert not ring_changed[:, 0].any() and not ring_changed[:, -1].any()                    # the corners and the closed west and east ring
    assert np.array_equal(after[0], patched[0]) and np.array_equal(after[-1], patched[-1])   # ... and they hold what the restatement imposed
    assert (rec["active"] == 1).all() and (rec["volume"] > 0).all()


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math_mode", [hp.MATH_FAST, hp.MATH_STRICT], ids=["fast", "strict"])
def test_save_and_restore_carry_the_records(math_mode):
    dom = make(math_mode)[0]
    add_all(dom)
    dom.step_batch(5)
    dom.state_save()
    dom.step_batch(15)
    device = lambda sc: {k: v for k, v in sc.items() if k not in ("cells_calculated", "iterations")}      # (the host's own counts run on)
    first = (dom.download(), device(dom.read_scalars()), dom.open_read())
    assert int(first[2]["active"].sum()) > 20
    dom.state_restore()
    dom.step_batch(15)
    again = (dom.download(), device(dom.read_scalars()), dom.open_read())
    assert np.array_equal(first[0], again[0]) and first[1] == again[1] and same_records(first[2], again[2])
    # a segment added since the snapshot voids its records: zero, and one warning
    lines = []
    hp.set_log_sink(lambda level, text: lines.append((level, text)))
    try:
        dom.add_open([dict(edge="south", first=25, last=30)])
        assert same_records(dom.open_read()[:36], again[2])                    # (the records there are move over to the larger block)
        dom.state_restore()
        rec = dom.open_read()
    finally:
        hp.set_log_sink(None)
    assert len(rec) == 42 and same_records(rec, np.zeros(42, hp.OPEN_RECORD_DTYPE))
    warnings = [text for level, text in lines if level == 8]
    assert len(warnings) == 1 and "open segments were added or cleared" in warnings[0], lines
    dom.step_batch(3)
    assert int(dom.open_read()["active"].sum()) > 0
    dom.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_errors_through_the_abi():
    pack = lambda s: hp.pack_open_segments(s, COLS, ROWS)
    for scheme in (hp.SCHEME_MUSCL_HANCOCK, hp.SCHEME_INERTIAL):
        dom = make(hp.MATH_FAST, scheme=scheme)[0]
        seg = pack(O.SEGMENTS)
        assert dom.lib.hp_boundary_add_open(dom.h, seg.ctypes.data_as(C.c_void_p), len(seg)) == -4        # HP_ERR_UNSUPPORTED
        assert "scheme" in dom.lib.hp_last_error().decode() and dom.open_info() == dict(segments=0, cells=0)
        dom.close()
    dom, st, bed, man = make(hp.MATH_FAST)
    lib = dom.lib

    def raw(segments, count=None):
        a = np.array([tuple(s) for s in segments], hp.OPEN_SEGMENT_DTYPE)
        return lib.hp_boundary_add_open(dom.h, a.ctypes.data_as(C.c_void_p), len(a) if count is None else count)
    for name, (segment, word) in O.BAD.items():
        assert raw([O.GOOD, segment]) == -1, name                              # HP_ERR_INVALID
        assert word in lib.hp_last_error().decode() and "segment 1" in lib.hp_last_error().decode(), (name, lib.hp_last_error())
    assert lib.hp_boundary_add_open(dom.h, None, 1) == -1 and raw([O.GOOD], 0) == -1 and lib.hp_boundary_add_open(None, None, 0) == -1
    assert raw([(O.SOUTH, 0, k, k) for k in range(1, 38)] + [(O.NORTH, 0, k, k) for k in range(1, 29)]) == -1      # 65 at once
    dom.step_begin()
    assert raw([O.GOOD]) == -5                                                 # HP_ERR_STATE inside a split step
    dom.step_end()
    assert dom.open_info() == dict(segments=0, cells=0)
    rec = np.zeros(1, hp.OPEN_RECORD_DTYPE)
    assert lib.hp_open_read(dom.h, 0, 1, rec.ctypes.data_as(C.c_void_p)) == -1 and lib.hp_open_read(dom.h, 0, 0, None) == 0
    # the domain is as usable as before: 64 segments, the 65th refused; a repeated cell over two calls names its id
    assert raw([(O.SOUTH, 0, k, k) for k in range(3, 19)]) == 0 and raw([(O.EAST, 0, k, k) for k in range(6, 26)]) == 0
    assert raw([(O.NORTH, 0, k, k) for k in range(1, 29)]) == 0 and dom.open_info() == dict(segments=64, cells=64)
    assert raw([(O.WEST, 0, 5, 5)]) == -1 and "64 segments" in lib.hp_last_error().decode()
    dom.clear_boundaries()
    assert dom.open_info() == dict(segments=0, cells=0)
    dom.add_open(O.SEGMENTS)
    assert raw([(O.EAST, 0, 25, 27)]) == -1 and f"cell {25 * COLS + COLS - 1} " in lib.hp_last_error().decode()
    assert dom.open_info() == dict(segments=2, cells=36)
    dom.step_batch(5)
    assert int(dom.open_read()["active"].sum()) > 0 and np.isfinite(dom.download()).all()
    # hp_boundary_clear removes it: the next batch changes no ring cell
    dom.clear_boundaries()
    assert dom.open_info() == dict(segments=0, cells=0)
    before = dom.download()
    dom.step_batch(4)
    after = dom.download()
    ring = np.ones((ROWS, COLS), bool)
    ring[1:-1, 1:-1] = False
    assert np.array_equal(after[ring], before[ring]) and not np.array_equal(after, before)
    dom.add_open(O.SEGMENTS)                                                   # the cells are free again
    assert same_records(dom.open_read(), np.zeros(36, hp.OPEN_RECORD_DTYPE))
    dom.close()


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_strips():
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", lib,
                               os.path.join(os.path.dirname(lib), "fake_rccl.cpp")])
    res = subprocess.run([sys.executable, os.path.join(HERE, "open_strips_worker.py"), "2"], capture_output=True, text=True, timeout=300)
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "FAILED" not in res.stdout and "the strips are the single domain True" in res.stdout


def test_strip_runner_gathers_the_records_of_the_hip_engine():
    """StripRunner over the HIP engine itself (HipEngine.add_open, HipEngine.open_read, StripRunner.gather_open), one strip: the
    gathered records are the single domain's in every bit."""
    single, st, bed, man = make(hp.MATH_STRICT)
    single.add_open(O.SEGMENTS[:1])
    single.add_open(O.SEGMENTS[1:])
    single.step_batch(20)
    want = single.open_read()
    single.close()
    runner = strips.StripRunner(COLS, ROWS, rank=0, world=1, backend="gloo", init_process_group=False, loop="torch", exchange_period=1,
                                dx=DX, math_mode=hp.MATH_STRICT)
    runner.upload_global(st, bed, man)
    runner.set_target_time(1e9)
    runner.add_open(O.SEGMENTS[:1])
    runner.add_open(O.SEGMENTS[1:])
    runner.domain.step_batch(20)
    got = runner.gather_open()
    assert got.dtype == hp.OPEN_RECORD_DTYPE and same_records(got, want) and int(want["active"].sum()) > 20
    assert same_records(runner.engine.open_read(first=20), want[20:])
    runner.engine.close()


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_the_tracer_leaves_with_the_water():
    """A plume beside the south outlet: M after 40 iterations is frontend.Tracer.apply run in the same loop behind Open.apply, in every
    bit, and the solute that flowed out has left the sum."""
    st, bed, man = O.scene()
    m0 = np.zeros((ROWS, COLS))
    m0[1:4, 6:12] = 2.0
    fn = oracle.OracleFunctions("f64", dx=DX)
    R = frontend.Open(ROWS, COLS, DX, fn, O.SEGMENTS)
    tracer = frontend.Tracer(ROWS, COLS, DX, fn, initial=m0)

    class Behind:                                          # the tracer's step behind every boundary, with the loop's own time
        def apply(self, state, b, dt):
            tracer.apply(state, b, dt, loop.sc.t)
    loop = T.StepLoop(st, bed, man, [("open", R), ("tracer", Behind())])
    loop.step(40)
    dom = make(hp.MATH_STRICT)[0]
    dom.add_open(O.SEGMENTS)
    dom.tracer_enable(m0)
    dom.step_batch(40)
    M = dom.tracer_read()
    assert np.array_equal(dom.download(), loop.download()) and same_records(dom.open_read(), R.records())
    assert np.array_equal(M, tracer.M)
    print("sum(M) before", float(m0.sum()), "after", float(M.sum()))
    assert M.sum() < m0.sum() - 1e-3
    dom.close()


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_model_writes_the_outflow(tmp_path):
    from hipims_mi.model import Model
    m = Model(O.write_model(tmp_path), output_format=".npy")
    m.run()
    rows = open(tmp_path / "out" / "outflow.csv").read().strip().split("\n")
    assert rows[0] == "t,discharge_outlet,volume_outlet,discharge_south1,volume_south1" and len(rows) >= 3
    rec = m.sim.open_read()
    assert m.sim.open_info() == dict(segments=2, cells=6 + 14)
    last = [float(v) for v in rows[-1].split(",")]
    assert last[2] == math.fsum(rec["volume"][:6]) and last[4] == math.fsum(rec["volume"][6:]) and last[2] > 0 and last[4] > 0
    assert last[2] + last[4] == math.fsum([math.fsum(rec["volume"][:6]), math.fsum(rec["volume"][6:])])
