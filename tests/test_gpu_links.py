"""Link groups on the GPU (hp_boundary_add_links; csrc/hp_links.hpp: bdy_links).  The reference is the stepwise loop over the
oracle's grid functions with frontend.Links.apply on the source buffer where the engine launches bdy_links (tests/test_links.py:
StepLoop, scene); STRICT runs and the links' records are compared bit for bit, FAST fp64 at the project's FAST tolerance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hipims_mi as hp
import oracle
import test_links as T
from hipims_mi import frontend, strips

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES = [1, 7, 20, 1, 7, 20, 1, 7, 20, 1, 7, 20, 1, 7]          # 120 iterations in batches of 1, 7 and 20


def same_records(got, want):
    return got.tobytes() == want.tobytes()


def same_scalars(sc, sr):
    return (sc["time"] == sr["t"] and sc["timestep"] == sr["dt"] and sc["time_hydrological"] == sr["t_hydro"] and sc["batch_timesteps"] == sr["batch_dt"]
            and sc["batch_successful"] == sr["batch_ok"] and sc["batch_skipped"] == sr["batch_skipped"])


def make(math_mode=hp.MATH_STRICT, precision="f64", scheme=hp.SCHEME_GODUNOV, all_wet=False):
    st, bed, man, links = T.scene(np.float64 if precision == "f64" else np.float32, all_wet=all_wet)
    dom = hp.Domain(T.COLS, T.ROWS, dx=T.DX, scheme=scheme, precision=precision, math_mode=math_mode)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    return dom, st, bed, man, links


def add_all(dom, links):
    """A uniform rain in front of the links and a cell boundary behind them."""
    dom.add_uniform(T.RAIN["definition"], T.RAIN["series"], T.RAIN["interval"], T.RAIN["length"])
    dom.add_links(links)
    dom.add_cell(T.INFLOW["depth_def"], T.INFLOW["discharge_def"], T.INFLOW["cells"], T.INFLOW["series"], T.INFLOW["interval"], T.INFLOW["length"])


@pytest.fixture(scope="module")
def reference():
    """The reference trajectory, computed once: (state, scalars, records) after every batch, and the branches taken."""
    assert sum(BATCHES) == 120
    st, bed, man, links = T.scene()
    # first: the loop WITHOUT links is the oracle's own run in every bit
    plain = T.StepLoop(st, bed, man, [("uniform", T.RAIN), ("cell", T.INFLOW)])
    ref = oracle.OracleSim(T.COLS, T.ROWS, dx=T.DX)
    ref.upload(st, bed, man)
    ref.add_uniform(T.RAIN["definition"], T.RAIN["series"], T.RAIN["interval"], T.RAIN["length"])
    ref.add_cell(T.INFLOW["depth_def"], T.INFLOW["discharge_def"], T.INFLOW["cells"], T.INFLOW["series"], T.INFLOW["interval"], T.INFLOW["length"])
    ref.set_target(1e9)
    plain.step(30)
    ref.run(30)
    assert np.array_equal(plain.download(), ref.download()) and plain.scalars() == ref.scalars()
    L = frontend.Links(T.ROWS, T.COLS, T.DX, links)
    loop = T.StepLoop(st, bed, man, [("uniform", T.RAIN), ("links", L), ("cell", T.INFLOW)])
    out = []
    for n in BATCHES:
        loop.step(n)
        out.append((loop.download(), loop.scalars(), L.records()))
    totals = L.branch_totals()
    assert all(totals[b] >= 1 for b in T.REQUIRED), totals
    return out, bed


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_strict_trajectory_is_the_reference_in_every_bit(reference):
    want, _ = reference
    dom, _, _, _, links = make(hp.MATH_STRICT)
    add_all(dom, links)
    assert not dom.boundaries_fused() and dom.links_info() == dict(links=8, groups=1)
    for k, n in enumerate(BATCHES):
        dom.step_batch(n)
        state, sc, rec = want[k]
        assert np.array_equal(dom.download(), state), f"state after batch {k}"
        assert same_scalars(dom.read_scalars(), sc), (k, dom.read_scalars(), sc)
        got = dom.links_read()
        assert same_records(got, rec), (k, got, rec)
    assert dom.pair_stats()["pairs"] == 0
    dom.close()


def test_fast_trajectory_is_within_the_fast_tolerance(reference):
    want, bed = reference
    dom, _, _, _, links = make(hp.MATH_FAST)
    add_all(dom, links)
    for k, n in enumerate(BATCHES):
        dom.step_batch(n)
        state, sc, rec = want[k]
        got = dom.download()
        wet = bed <= 9999.0
        rmse = float(np.sqrt(np.mean(((got[..., 0] - state[..., 0])[wet]) ** 2)))
        print("batch", k, "depth RMSE", rmse)
        assert rmse < 1e-9, (k, rmse)
        assert np.array_equal(dom.links_read()["active"], rec["active"]), k
    dom.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math_mode", [hp.MATH_FAST, hp.MATH_STRICT], ids=["fast", "strict"])
@pytest.mark.parametrize("scheme", [hp.SCHEME_GODUNOV, hp.SCHEME_INERTIAL], ids=["godunov", "inertial"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_one_iteration_is_its_twin(precision, scheme, math_mode):
    """All wet, so that no cell is left untouched by the flux kernel: a domain with the links against a fresh upload of the state the
    restatement has patched, one iteration each."""
    a, st, bed, man, links = make(math_mode, precision, scheme, all_wet=True)
    b = make(math_mode, precision, scheme, all_wet=True)[0]
    a.add_links(links)
    dt0 = a.read_scalars()["timestep"]
    L = frontend.Links(T.ROWS, T.COLS, T.DX, links)
    patched = st.copy()
    assert L.apply(patched, bed, dt0) >= 5 and not np.array_equal(patched, st)
    b.upload(state=patched)
    a.step_batch(1)
    b.step_batch(1)
    assert np.array_equal(a.download(), b.download())
    assert a.read_scalars() == b.read_scalars()
    assert same_records(a.links_read(), L.records()), (a.links_read(), L.records())
    a.close(); b.close()


def test_links_are_inert_under_muscl_hancock():
    a, st, bed, man, links = make(hp.MATH_FAST, "f64", hp.SCHEME_MUSCL_HANCOCK, all_wet=True)
    b = make(hp.MATH_FAST, "f64", hp.SCHEME_MUSCL_HANCOCK, all_wet=True)[0]
    a.add_links([l for l in links if min(l["a"][1], l["b"][1]) >= 2])
    a.step_batch(4); b.step_batch(4)
    assert np.array_equal(a.download(), b.download()) and int(a.links_read()["active"].sum()) == 0
    a.close(); b.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_no_pairs_with_links():
    res = subprocess.run([sys.executable, os.path.join(HERE, "links_pairs_worker.py")], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, HP_TWO_STEP="1"))
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "no pairs with links, pairs without" in res.stdout


def test_a_domain_with_links_never_speculates():
    clean = {k: v for k, v in os.environ.items() if k not in ("HP_STRICT_SPECULATE", "HP_STRICT_SPEC_FORCE")}
    res = subprocess.run([sys.executable, os.path.join(HERE, "links_spec_worker.py")], capture_output=True, text=True, timeout=300,
                         env=dict(clean, HP_STRICT_SPECULATE="1", HP_STRICT_SPEC_FORCE="1"))
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "a domain with links never speculates" in res.stdout


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math_mode", [hp.MATH_FAST, hp.MATH_STRICT], ids=["fast", "strict"])
def test_save_and_restore_carry_the_records(math_mode):
    dom, _, _, _, links = make(math_mode)
    add_all(dom, links)
    dom.step_batch(5)
    dom.state_save()
    dom.step_batch(10)
    device = lambda sc: {k: v for k, v in sc.items() if k not in ("cells_calculated", "iterations")}      # (the host's own counts run on)
    first = (dom.download(), device(dom.read_scalars()), dom.links_read())
    assert int(first[2]["active"].sum()) > 20
    dom.state_restore()
    dom.step_batch(10)
    again = (dom.download(), device(dom.read_scalars()), dom.links_read())
    assert np.array_equal(first[0], again[0]) and first[1] == again[1] and same_records(first[2], again[2])
    # a group added since the snapshot voids its records: zero, and one warning
    lines = []
    hp.set_log_sink(lambda level, text: lines.append((level, text)))
    try:
        dom.add_links([dict(a=(5, 12), b=(30, 12), kind=T.PUMP, level=0.0, size=0.1)])
        dom.state_restore()
        rec = dom.links_read()
    finally:
        hp.set_log_sink(None)
    assert len(rec) == 9 and same_records(rec, np.zeros(9, hp.LINK_RECORD_DTYPE))
    warnings = [text for level, text in lines if level == 8]
    assert len(warnings) == 1 and "link groups were added or cleared" in warnings[0], lines
    dom.step_batch(3)
    assert int(dom.links_read()["active"].sum()) > 0
    dom.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reaches", [1, 2])
@pytest.mark.parametrize("world", [2, 3])
def test_strips(world, reaches):
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", lib,
                               os.path.join(os.path.dirname(lib), "fake_rccl.cpp")])
    res = subprocess.run([sys.executable, os.path.join(HERE, "links_strips_worker.py"), str(world), str(reaches)], capture_output=True, text=True, timeout=300)
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "FAILED" not in res.stdout and "the strips are the single domain True" in res.stdout


def test_strip_runner_gathers_the_records_of_the_hip_engine():
    """StripRunner over the HIP engine itself (HipEngine.add_links, HipEngine.links_read, StripRunner.gather_links), one strip:
    the gathered records are the single domain's in every bit."""
    st, bed, man, links = T.scene()
    single, _, _, _, _ = make(hp.MATH_STRICT)
    single.add_links(links[:5])
    single.add_links(links[5:])
    single.step_batch(20)
    want = single.links_read()
    single.close()
    runner = strips.StripRunner(T.COLS, T.ROWS, rank=0, world=1, backend="gloo", init_process_group=False, loop="torch", exchange_period=1,
                                dx=T.DX, math_mode=hp.MATH_STRICT)
    runner.upload_global(st, bed, man)
    runner.set_target_time(1e9)
    runner.add_links(links[:5])
    runner.add_links(links[5:])
    runner.domain.step_batch(20)
    got = runner.gather_links()
    assert got.dtype == hp.LINK_RECORD_DTYPE and same_records(got, want) and int(want["active"].sum()) > 20
    assert same_records(runner.engine.links_read(first=5), want[5:])
    runner.engine.close()


@pytest.mark.parametrize("reaches", [1, 2])
def test_a_strip_with_one_end_is_refused_before_any_rank_adds(reaches):
    g = strips.ghost_rows(hp.SCHEME_GODUNOV) * reaches
    parts = strips.partition(T.ROWS, 2, g)
    st, bed, man, links = T.scene()
    cut = parts[0][1]
    across = dict(a=(5, cut - 5), b=(9, cut + 5), kind=T.WEIR, level=1.0, size=1.0, coeff=1.7, limit=0.5)

    class Engine:                                          # rank 0's strip, a real domain
        def __init__(self, cols, local_rows, global_rows, row_offset):
            lo, hi = parts[0][2], parts[0][3]              # (the rows of THIS test's partition: the runner's own has one reach)
            self.domain = hp.Domain(cols, hi - lo, dx=T.DX, global_rows=global_rows, row_offset=lo, ghost_rows=g if reaches > 1 else 0)
            self.domain.upload(st[lo:hi], bed[lo:hi], man[lo:hi])

        def add_links(self, l):
            self.domain.add_links(l)
    runner = strips.StripRunner(T.COLS, T.ROWS, rank=0, world=2, engine_factory=Engine, init_process_group=False, loop="torch", exchange_period=1)
    runner.parts = parts
    with pytest.raises(ValueError, match="link 8 "):
        runner.add_links(links + [across])
    dom = runner.engine.domain
    assert dom.links_info() == dict(links=0, groups=0)
    # the library refuses the same link by itself, names it, and stays usable
    with pytest.raises(hp.HipimsError, match="link 8 ") as e:
        dom.add_links(links + [across])
    assert dom.lib.hp_boundary_add_links(dom.h, hp.pack_links([across], T.COLS).ctypes.data_as(C.c_void_p), 1) == -4         # HP_ERR_UNSUPPORTED
    if reaches == 2:                                       # an end on the outermost reach of ghost rows, the other on a row that is always valid
        lo, hi = parts[0][2], parts[0][3]
        assert dom.lib.hp_boundary_add_links(dom.h, hp.pack_links([dict(across, a=(5, hi - 1), b=(9, hi - 2))], T.COLS).ctypes.data_as(C.c_void_p), 1) == -4
    assert dom.links_info() == dict(links=0, groups=0)
    dom.add_links(links)
    dom.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_through_the_abi():
    dom, _, _, _, links = make(hp.MATH_FAST)
    lib = dom.lib
    raw = lambda l, count=None: lib.hp_boundary_add_links(dom.h, hp.pack_links(l, T.COLS).ctypes.data_as(C.c_void_p), len(l) if count is None else count)
    for name, (link, word) in T.BAD.items():
        assert raw([T.GOOD, link] if name != "a == b" else [link]) == -1, name
        assert word in lib.hp_last_error().decode(), (name, lib.hp_last_error())
    assert lib.hp_boundary_add_links(dom.h, None, 1) == -1 and raw([T.GOOD], 0) == -1 and raw([T.GOOD], 65537) == -1
    assert raw([T.GOOD, dict(T.GOOD, a=(7, 7), b=(9, 9))]) == -1 and f"cell {9 * T.COLS + 9} " in lib.hp_last_error().decode()
    assert lib.hp_boundary_add_links(None, None, 0) == -1
    dom.step_begin()
    assert raw([T.GOOD]) == -5                             # HP_ERR_STATE inside a split step
    dom.step_end()
    assert dom.links_info() == dict(links=0, groups=0)
    rec = np.zeros(1, hp.LINK_RECORD_DTYPE)
    assert lib.hp_links_read(dom.h, 0, 1, rec.ctypes.data_as(C.c_void_p)) == -1 and lib.hp_links_read(dom.h, 0, 0, None) == 0
    # the domain is as usable as before: the scene's links, then a repeated cell over two groups
    dom.add_links(links)
    assert raw([dict(T.GOOD, a=(18, 6), b=(30, 6))]) == -1 and f"cell {6 * T.COLS + 18} " in lib.hp_last_error().decode()
    assert dom.links_info() == dict(links=8, groups=1)
    dom.step_batch(5)
    assert int(dom.links_read()["active"].sum()) > 0 and np.isfinite(dom.download()).all()
    dom.clear_boundaries()
    assert dom.links_info() == dict(links=0, groups=0)
    dom.add_links([T.GOOD])                                # the cells are free again
    dom.close()
