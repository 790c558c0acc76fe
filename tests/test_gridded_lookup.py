"""Gridded boundaries at non-zero offsets and uneven resolutions, without a GPU.

1. The cover check of hp_boundary_add_gridded (csrc/hp_gridded.hpp, through the stand-alone program tests/gridded_probe.cpp) against a
   NumPy restatement that evaluates the lookup at EVERY interior cell in the domain's precision: three counter-examples that a check in
   double let through for fp32 domains, and a seeded sweep.
2. The oracle's lookup (orc_bdy_gridded, called on a state array as host_calls_actors.StepTwin calls the grid functions) against an
   independent restatement, bit for bit, over the table of tests/gridded_cases.py.
3. The oracle's simulation against the reference build's bdy_Gridded over the same table (where oracle/_ref is built).
The oracle has no range check at all: every grid handed to it here is one the fixed check accepts."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import gridded_cases as gc
import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hipims-ocl_amd", "csrc")
REALS = {"f32": np.float32, "f64": np.float64}

# (dx, resolution, cols, off_x, grid_cols): the double quotient at x = cols - 2 stays below grid_cols, the float quotient reaches it
COUNTER_EXAMPLES = [(0.3, 10.0, 103, 0.3, 3), (1.1, 1.1, 267, 1.1, 264), (0.7, 28.0, 41, -0.7, 1)]


def bits(v):
    return struct.pack(">d", float(v)).hex()


def line(dx, res, ox, oy, cols, rows, gcols, grows):
    return f"{bits(dx)} {bits(res)} {bits(ox)} {bits(oy)} {cols} {rows} {gcols} {grows}"


def build_probe(exe, *flags):
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, "-I", CSRC, "-o", str(exe), os.path.join(HERE, "gridded_probe.cpp")],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gridded") / "gridded_probe"
    r = build_probe(exe, "-O2")
    assert r.returncode == 0, r.stderr[-2000:]

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == len(lines)
        return [(o[0] == "1", o[1] == "1") for o in out]                      # (fp32 verdict, fp64 verdict)
    return run


def restated(real, dx, res, ox, oy, cols, rows, gcols, grows):
    return gc.covers(real, cols, dx, ox, res, gcols) and gc.covers(real, rows, dx, oy, res, grows)


def test_the_cover_check_needs_no_hip():
    text = open(os.path.join(CSRC, "hp_gridded.hpp")).read()
    assert "hip_runtime" not in text and "__global__" not in text
    assert '#include "hp_gridded.hpp"' in open(os.path.join(CSRC, "hp_actors.hpp")).read()
    assert "hp_gridded.hpp" in open(os.path.join(CSRC, "Makefile")).read()


def test_counter_examples_are_refused_in_fp32_and_taken_in_fp64(probe):
    """Along x, and the same numbers along y (rows for columns): the grid's other axis is a plain 8 dx grid that covers."""
    lines, want = [], []
    for dx, res, n, off, cells in COUNTER_EXAMPLES:
        other = int(np.ceil(40 * dx / res)) + 1
        lines += [line(dx, res, off, 0.0, n, 40, cells, other), line(dx, res, 0.0, off, 40, n, other, cells)]
        for real in (np.float32, np.float64):                                 # what the restatement says of them, first
            assert gc.covers(real, 40, dx, 0.0, res, other)
            assert gc.covers(real, n, dx, off, res, cells) == (real is np.float64), (dx, res, n, off, cells)
        q64 = (np.float64(n - 2) * dx - off) / res
        q32 = (np.float32(n - 2) * np.float32(dx) - np.float32(off)) / np.float32(res)
        assert cells - 1e-9 < q64 < cells <= float(q32) < cells + 1e-4       # just below the grid's end in double, on it or past it in float
        want += [(False, True)] * 2
    assert probe(lines) == want
    # one more grid cell along that axis and both take it
    assert probe([line(dx, res, off, 0.0, n, 40, cells + 1, int(np.ceil(40 * dx / res)) + 1) for dx, res, n, off, cells in COUNTER_EXAMPLES]) == [(True, True)] * 3


def sweep(count=24000, seed=20250611):
    """Plain dx, resolution and offset values; half of the draws put the last interior coordinate ON a grid line (where the two
    precisions can part); the grid is the smallest one a check in double accepts, sometimes one cell smaller or larger."""
    rng = np.random.default_rng(seed)
    plain = np.round(np.concatenate([np.arange(1, 31) * 0.1, [0.25, 0.5, 1.0, 2.0, 5.0, 7.5, 10.0, 20.0, 40.0]]), 10)
    out = []
    for _ in range(count):
        dx = float(rng.choice(plain))
        m = int(rng.choice([1, 2, 3, 7, 8, 10, 33, 40, 64, 100]))
        res = float(rng.choice([dx * m, round(dx * m, 6), float(rng.choice(plain)) * m, round(dx * rng.uniform(1, 70), 2)]))
        axes = []
        for _axis in range(2):
            j = int(rng.choice([1, 1, 0, -1, -2, -5]))
            off = float(rng.choice([j * dx, dx / 2, 0.0, -0.37 * res, -res, dx * 1.0000001, round(rng.uniform(-2, 1) * dx, 3)]))
            if rng.random() < 0.5:
                n = j + 2 + m * int(rng.integers(1, max(2, 400 // m)))
            else:
                n = int(rng.integers(3, 420))
            n = max(3, n)
            idx = gc.indices(np.float64, n, dx, off, res)[1:n - 1]
            cells = max(1, int(idx.max()) + 1 + int(rng.choice([0, 0, 0, 0, -1, 1])))
            axes.append((off, n, cells))
        (ox, cols, gcols), (oy, rows, grows) = axes
        out.append((dx, res, ox, oy, cols, rows, gcols, grows))
    return out


def test_probe_equals_the_restatement_at_every_interior_cell_over_a_seeded_sweep(probe):
    draws = sweep()
    assert len(draws) >= 20000
    got = probe([line(*d) for d in draws])
    part = taken = refused = 0
    for d, (g32, g64) in zip(draws, got):
        w32, w64 = restated(np.float32, *d), restated(np.float64, *d)
        assert (g32, g64) == (w32, w64), (d, (g32, g64), (w32, w64))
        part += w32 != w64
        taken += w64
        refused += not w64
    print(f"sweep: {len(draws)} draws, fp64 takes {taken} and refuses {refused}; fp32 and fp64 part on {part}")
    assert part >= 10 and taken >= 1000 and refused >= 1000                  # the sweep is not vacuous


def test_fp64_verdict_is_the_former_check(probe):
    """For an fp64 domain the decision is the one hp_boundary_add_gridded made before the check moved: the same comparisons in double."""
    draws = sweep(count=6000, seed=77)
    got = probe([line(*d) for d in draws])
    for (dx, res, ox, oy, cols, rows, gcols, grows), (_, g64) in zip(draws, got):
        x_lo, x_hi = 1.0 * dx - ox, float(cols - 2) * dx - ox
        y_lo, y_hi = 1.0 * dx - oy, float(rows - 2) * dx - oy
        former = not (x_lo < 0.0 or y_lo < 0.0 or np.floor(x_hi / res) >= float(gcols) or np.floor(y_hi / res) >= float(grows))
        assert g64 == former, (dx, res, ox, oy, cols, rows, gcols, grows)


def test_the_probe_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Host code with its own main: built with the sanitizers and run on its own."""
    exe = tmp_path / "gridded_probe_san"
    r = build_probe(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if r.returncode != 0 and "asan" in r.stderr.lower() + r.stdout.lower():
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    draws = sweep(count=300, seed=5)
    lines = [line(dx, res, off, 0.0, n, 40, cells, 40) for dx, res, n, off, cells in COUNTER_EXAMPLES] + [line(*d) for d in draws]
    lines.append(line(1.0, 1e-300, -1e300, 1e300, 2 ** 40, 3, 2 ** 63, 1))   # indices far beyond any integer type: compared as floating point
    res = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-2000:]
    out = res.stdout.split()
    assert out[:3] == ["01"] * 3 and len(out) == len(lines) and out[-1] == "00"


def test_the_table_is_what_it_says():
    """64 dx and 66.7 dx are at or above the fusion threshold `resolution < 64 dx` (evaluated in double, csrc/hp_actors.hpp), 63.99 dx is
    below; (dx, dx) puts row and column 0 at index -1; the uneven rows put grid lines off the multiples of 64 cells."""
    for dx in gc.DXS:
        for real in REALS.values():
            rows = gc.table(dx, real)
            assert len(rows) == 50 and len({r[0] for r in rows}) == 50
            for label, res, ox, oy, gr, gcols in rows:
                assert gc.covers(real, gc.COLS, dx, ox, res, gcols) and gc.covers(real, gc.ROWS, dx, oy, res, gr), label
                if label.endswith("min"):
                    assert not gc.covers(real, gc.COLS, dx, ox, res, gcols - 1) and not gc.covers(real, gc.ROWS, dx, oy, res, gr - 1), label
        assert not (64.0 * dx < 64.0 * dx) and not (66.7 * dx < 64.0 * dx) and 63.99 * dx < 64.0 * dx
        for real in REALS.values():
            assert gc.indices(real, 3, dx, dx, 64 * dx)[0] == -1 and gc.indices(real, 3, dx, dx, 64 * dx)[1] == 0
    # an uneven coarse row: a grid line inside the domain, away from a multiple of 64 cells, along both axes
    cx = gc.indices(np.float64, gc.COLS, 40.0, -0.37 * 66.7 * 40.0, 66.7 * 40.0)
    cy = gc.indices(np.float64, gc.ROWS, 40.0, -0.61 * 66.7 * 40.0, 66.7 * 40.0)
    assert [int(k) for k in np.flatnonzero(np.diff(cx)) + 1] == [43, 109, 176] and [int(k) for k in np.flatnonzero(np.diff(cy)) + 1] == [27, 93]


# 2 ---------------------------------------------------------------------------------------------------------------------
def scene_with_nulls(real):
    st, bed, man = gc.scene(real)
    st[30, 44, 1] = -9999.0                                 # Zmax disabled
    st[60, 110, 0] = -9999.0                                # level disabled
    st[27, 43, 0] = st[27, 43, 1] = -9999.0                 # both, on a grid corner of the uneven rows
    return st, bed, man


@pytest.mark.parametrize("dx", gc.DXS)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_oracle_lookup_equals_an_independent_restatement_bit_for_bit(precision, dx):
    """orc_bdy_gridded on a state array with t_hydro >= 1: the level of every cell afterwards is level + increment with row, column
    and slice restated per cell in the domain's precision -- every table row, both definitions, the NDRange whole and truncated (Q9),
    the three slices and the clamp behind the last."""
    real = REALS[precision]
    sim = oracle.OracleSim(gc.COLS, gc.ROWS, dx=dx, precision=precision)
    lib, p, r = sim.lib, C.byref(sim.p), sim.creal
    st0, bed, _ = scene_with_nulls(real)
    y, x = np.mgrid[0:gc.ROWS, 0:gc.COLS]
    interior = (x >= 1) & (x <= gc.COLS - 2) & (y >= 1) & (y <= gc.ROWS - 2)
    live = ~((st0[..., 1] <= real(-9999.0)) | (st0[..., 0] == real(-9999.0)))
    checked = 0
    for label, res, ox, oy, gr, gcols in gc.table(dx, real):
        for definition in gc.DEFINITIONS:
            grids = gc.rates(definition, gc.SLICES, gr, gcols, real)
            for truncated in (0, 1):
                for t, th in ((0.0, 1.0), (gc.T0, 6.25), (2 * gc.INTERVAL + 3.0, 1.5), (5 * gc.INTERVAL, 3.0)):
                    sc = sim.Scalars(t=t, dt=th, t_hydro=th, t_sync=1e9, batch_dt=0.0, batch_ok=0, batch_skipped=0)
                    st = st0.copy()
                    lib.orc_bdy_gridded(p, C.byref(sc), definition, oracle._ptr(grids), C.c_ulong(gc.SLICES), C.c_ulong(gr), C.c_ulong(gcols),
                                        r(res), r(ox), r(oy), r(gc.INTERVAL), oracle._ptr(st), oracle._ptr(bed), C.c_int(truncated))
                    ts = min(int(np.floor(real(t) / real(gc.INTERVAL))), gc.SLICES - 1)
                    inc, ok = gc.increment(real, definition, grids, ts, dx, res, ox, oy, th)
                    hit = interior & live
                    if truncated:
                        hit = hit & (x < (gc.COLS // 8) * 8) & (y < (gc.ROWS // 8) * 8)
                    assert ok[hit].all(), label
                    want = st0.copy()
                    want[..., 0] = np.where(hit, st0[..., 0] + inc, st0[..., 0])
                    assert np.array_equal(st.view(np.uint8), want.view(np.uint8)), (label, definition, truncated, t)
                    assert (inc[hit] > 0).all() and np.isfinite(st).all()
                    checked += 1
    assert checked == 50 * 2 * 2 * 4
    # below the hydrological gate nothing is applied
    sc = sim.Scalars(t=gc.T0, dt=0.5, t_hydro=0.999, t_sync=1e9, batch_dt=0.0, batch_ok=0, batch_skipped=0)
    st = st0.copy()
    lib.orc_bdy_gridded(p, C.byref(sc), 0, oracle._ptr(grids), C.c_ulong(gc.SLICES), C.c_ulong(gr), C.c_ulong(gcols), r(res), r(ox), r(oy),
                        r(gc.INTERVAL), oracle._ptr(st), oracle._ptr(bed), C.c_int(0))
    assert np.array_equal(st, st0)


def run_plan(sim, plan=gc.PLAN):
    out = []
    for step in plan:
        if step == "download":
            sim.download()
        else:
            sim.run(step)
            out.append((sim.download(), sim.scalars()))
    return out


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_oracle_stays_finite_and_rains_on_every_case_of_the_gpu_tests(precision):
    """What tests/test_gpu_gridded_lookup.py holds the engines to: the oracle's run of the plan on every table row at dx = 40 is
    finite, the gate is open from the second iteration on, the time slice changes inside the run, and the rain reaches dry land."""
    real = REALS[precision]
    st, bed, man = gc.scene(real)
    for label, res, ox, oy, gr, gcols in gc.table(40.0, real):
        for definition in gc.DEFINITIONS:
            sim = oracle.OracleSim(gc.COLS, gc.ROWS, dx=40.0, precision=precision, dt_initial=gc.DT0)
            sim.upload(st, bed, man)
            sim.add_gridded(definition, gc.rates(definition, gc.SLICES, gr, gcols, real), res, ox, oy, gc.INTERVAL)
            sim.set_time(gc.T0)
            sim.set_target(1e9)
            batches = run_plan(sim)
            for state, sc in batches:
                assert np.isfinite(state).all() and sc["t_hydro"] >= 1.0 and sc["dt"] >= 1.0, (label, definition, sc)
            t_first, t_last = batches[0][1]["t"], batches[-1][1]["t"]
            assert int(t_first // gc.INTERVAL) == 1 and int(t_last // gc.INTERVAL) >= 2, (label, t_first, t_last)
            dry0 = (st[..., 0] - bed)[1:-1, 1:-1] < 1e-6
            assert dry0.mean() > 0.5 and ((batches[-1][0][..., 0] - bed)[1:-1, 1:-1][dry0] > 1e-5).mean() > 0.5, label


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not oracle.have_ref(), reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("dx", gc.DXS)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_oracle_equals_the_reference_build_over_the_table(precision, dx):
    """The oracle's lookup pinned to the reference's own bdy_Gridded away from offset 0: both run the plan on every table row.  At
    dx = 40 as the GPU tests run it (the clock past the first minute, a first timestep of 2 s: rain from the second iteration on); at
    dx = 0.3 from the defaults, with iterations added until the hydrological time has passed a second (timesteps of 0.1 s and less)."""
    real = REALS[precision]
    cols, rows = 70, 37                                    # a small grid: two grid columns and rows of the coarse uneven rows, 9 x 5 of the fine ones
    st, bed, man = gc.scene(real, cols, rows)
    big = dx == 40.0
    plan = gc.PLAN if big else gc.PLAN + (30,)
    # behind the last slice the reference reads one slice PAST the grids (CLBoundaries.clc:229; the oracle and the engine clamp to the
    # last one): an interval with which the run changes slice once and ends inside the last (t = 70 .. 170 s at dx = 40)
    interval = 60.0
    for label, res, ox, oy, gr, gcols in gc.table(dx, real, cols=cols, rows=rows):
        for definition in gc.DEFINITIONS:
            grids = gc.rates(definition, gc.SLICES, gr, gcols, real)
            if not big and definition == 2:
                grids = grids * real(1e-4)                 # (a 0.3 m cell: the flux of a 40 m cell would stand metres high on it)
            kw = dict(dx=dx, precision=precision, dt_initial=gc.DT0 if big else 0.001)
            a, b = oracle.OracleSim(cols, rows, **kw), oracle.RefSim(cols, rows, **kw)
            for s in (a, b):
                s.upload(st, bed, man)
                s.add_gridded(definition, grids, res, ox, oy, interval)
                s.set_target(1e9)
            if big:
                a.set_time(gc.T0)
                b.t[0] = gc.T0
            runs = list(zip(run_plan(a, plan), run_plan(b, plan)))
            for (sa, ca), (sb, cb) in runs:
                assert np.array_equal(sa.view(np.uint8), sb.view(np.uint8)), (label, definition)
                assert ca == {k: type(ca[k])(v) for k, v in cb.items()}, (label, definition)
            assert not big or 2 * interval < runs[-1][0][1]["t"] < 3 * interval
            wetter = (runs[-1][0][0][..., 0] > st[..., 0])[1:rows // 8 * 8, 1:cols // 8 * 8]
            assert np.isfinite(runs[-1][0][0]).all() and wetter.mean() > 0.5, (label, definition)      # it rained, on both
