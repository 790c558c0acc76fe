"""Gridded boundaries at non-zero offsets and uneven resolutions on the GPU: the four places that restate the lookup
(bdy_gridded / bdy_area, the fused epilogue of godunov_march, the table of godunov_march2 with area boundaries, and the strips'
row_offset on top of them) held to the oracle over the table of tests/gridded_cases.py.

The domain: 190 x 101 cells of 40 m, mostly dry land with pools at rest; the clock set past the first minute and a first timestep of
2 s, so that the hydrological gate is open from the second iteration on; 1 + 2 + 5 + 4 iterations with a download in between; three
time slices of 45 s (the slice changes inside the run and the clamp behind the last one is reached); a distinct rate per grid cell.
Every path runs in a child process of its own (tests/gridded_lookup_worker.py: the environment switches are read once per process),
every table row that applies to it, rain intensity and mass flux, fp64 and fp32.

  STRICT  equals oracle.OracleSim in every bit of the state and of the time scalars after every batch, in every case.
  FAST    within the project's bounds of the oracle (fp64: depth RMSE < 1e-9 m, max < 1e-7 m, time relative < 1e-12; fp32: 1e-4 m);
          fused equals unfused (HP_FUSE_BDY=0) and pairs equal single iterations, bit for bit.
tests/test_gridded_lookup.py is the CPU check that the oracle stays finite, and rains, on each of these cases."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import gridded_cases as gc
import hipims_mi as hp
import oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = {
    "standalone": {}, "inertial": {}, "basic": {},
    "unfused": dict(HP_FUSE_BDY="0", HP_TWO_STEP="0"), "unfused_loss": dict(HP_FUSE_BDY="0", HP_TWO_STEP="0"),
    "k1": dict(HP_TWO_STEP="0"), "k1_loss": dict(HP_TWO_STEP="0"),
    "k1b": dict(HP_TWO_STEP="1"), "k1b_exact": dict(HP_TWO_STEP="1", HP_PAIR_EXACT="1"), "k1b_loss": dict(HP_TWO_STEP="1"),
}
FUSED = {"k1": True, "k1_loss": True, "k1b": True, "k1b_exact": True, "k1b_loss": True, "unfused": False, "unfused_loss": False,
         "standalone": False, "inertial": False, "basic": False}
# FAST runs iteration pairs (godunov_march2 with area boundaries) where HP_TWO_STEP=1 says so; STRICT runs no pairs on a domain with
# boundaries (hp_engine.hip, pairs_possible_common), its iterations there are godunov_march with the fused epilogue
PAIRS = {"k1b": True, "k1b_exact": True, "k1b_loss": True, "k1": False, "k1_loss": False, "unfused": False, "unfused_loss": False}
PRECISIONS = ["f64", "f32"]


@functools.lru_cache(maxsize=None)
def run_path(path, precision):
    """One child process per path and precision; its JSON (one entry per table row and definition), run once for all tests."""
    env = {k: v for k, v in os.environ.items() if k not in ("HP_FUSE_BDY", "HP_TWO_STEP", "HP_PAIR_EXACT")}
    env.update(ENV[path])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.json")
        res = subprocess.run([sys.executable, os.path.join(HERE, "gridded_lookup_worker.py"), path, precision, out], capture_output=True, text=True, env=env,
                             timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        print(res.stdout.strip())
        with open(out) as f:
            cases = json.load(f)
    rows = 2 * len(gc.table(40.0, np.float64, gc.RES_FINE if path == "standalone" else gc.RES_FUSED))
    assert len(cases) == rows and all(len(c["strict_equal"]) == 4 for c in cases)       # no case is skipped
    return cases


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("path", list(ENV))
def test_strict_equals_the_oracle_in_every_bit(path, precision):
    cases = run_path(path, precision)
    for c in cases:
        assert c["finite"], (c["label"], c["definition"])
        assert all(c["strict_equal"]), (path, precision, c["label"], c["definition"], c["first_diff"])
        assert c["strict_fused"] == FUSED[path] and c["fast_fused"] == FUSED[path], (path, c["label"])
        if path in PAIRS:
            assert c["strict_pairs"] == 0 and (c["fast_pairs"] > 0) == PAIRS[path], (path, c["label"], c["strict_pairs"], c["fast_pairs"])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("path", list(ENV))
def test_fast_is_within_the_projects_bounds_of_the_oracle(path, precision):
    """Measured on an MI355X, the largest over a path's cases and batches: fp64 depth RMSE 1.9e-16 m, max 1.4e-14 m, time 5.4e-16 (all
    twelve iterations of every row are inside the fp64 bounds: no plan was shortened); fp32 depth RMSE 9.7e-6 m, time 1.9e-7, and a
    largest single-cell difference of 9.5e-4 m, for which the project has no bound in fp32 (tests/test_gpu_parity.py)."""
    rmse_bar, max_bar, time_bar = (1e-9, 1e-7, 1e-12) if precision == "f64" else (1e-4, np.inf, 1e-5)
    cases = run_path(path, precision)
    print(f"{path} {precision}: depth RMSE up to {max(max(c['rmse']) for c in cases):.3e} m, max {max(max(c['max']) for c in cases):.3e} m, "
          f"time {max(max(c['time_rel']) for c in cases):.3e}")
    for c in cases:
        assert max(c["rmse"]) < rmse_bar and max(c["max"]) < max_bar and max(c["time_rel"]) <= time_bar, (path, precision, c["label"], c["definition"],
                                                                                                         c["rmse"], c["max"], c["time_rel"])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("a,b", [("k1", "unfused"), ("k1_loss", "unfused_loss"), ("k1b", "k1"), ("k1b_exact", "k1"), ("k1b_loss", "k1_loss")])
def test_fast_paths_equal_each_other_bit_for_bit(a, b, precision):
    """Fused against unfused, pairs against single iterations: the same state and time scalars after every batch."""
    for ca, cb in zip(run_path(a, precision), run_path(b, precision)):
        assert (ca["label"], ca["definition"]) == (cb["label"], cb["definition"])
        assert ca["digest"] == cb["digest"], (a, b, precision, ca["label"], ca["definition"])


def make(precision, math_mode=hp.MATH_FAST, cols=gc.COLS, rows=gc.ROWS, dx=40.0, **kw):
    real = np.float64 if precision == "f64" else np.float32
    dom = hp.Domain(cols, rows, dx=dx, precision=precision, math_mode=math_mode, **kw)
    dom.upload(*gc.scene(real, cols, rows))
    return dom, real


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fusion_threshold(precision):
    """A grid of 63.99 dx keeps the stand-alone pass, one of 64 dx rides in the flux kernel (`resolution < 64 dx`, in double)."""
    for cells, fused in ((63.99, False), (64.0, True), (66.7, True)):
        dom, real = make(precision)
        res = cells * 40.0
        gr, gcols = gc.smallest_grid(real, 40.0, res, 40.0, 40.0)
        dom.add_gridded(hp.GRIDDED_RAIN_INTENSITY, gc.rates(0, gc.SLICES, gr, gcols, real), res, 40.0, 40.0, gc.INTERVAL)
        assert dom.boundaries_fused() == fused, (cells, precision)
        dom.close()


# (dx, resolution, n, offset, grid cells along that axis): accepted by a check in double, out of range in float
COUNTER_EXAMPLES = [(0.3, 10.0, 103, 0.3, 3), (1.1, 1.1, 267, 1.1, 264), (0.7, 28.0, 41, -0.7, 1)]


@pytest.mark.parametrize("dx,res,n,off,cells", COUNTER_EXAMPLES)
def test_an_fp32_domain_refuses_what_its_kernels_would_read_out_of_range(dx, res, n, off, cells):
    """The float quotient at the last interior column reaches grid_cols: refused before anything is uploaded or launched.  The fp64
    domain takes the same call, and then matches the oracle."""
    rows = 40
    other = int(np.ceil(rows * dx / res)) + 1
    assert not gc.covers(np.float32, n, dx, off, res, cells) and gc.covers(np.float64, n, dx, off, res, cells)
    dom, real = make("f32", cols=n, rows=rows, dx=dx)
    before = dom.launch_counts()
    with pytest.raises(hp.HipimsError, match="gridded boundary does not cover the domain's interior cells"):
        dom.add_gridded(hp.GRIDDED_RAIN_INTENSITY, gc.rates(0, 2, other, cells, real), res, off, 0.0, 30.0)
    assert dom.launch_counts() == before and not dom.boundaries_fused()
    dom.add_gridded(hp.GRIDDED_RAIN_INTENSITY, gc.rates(0, 2, other, cells + 1, real), res, off, 0.0, 30.0)     # one more column covers
    dom.close()
    dom, real = make("f64", math_mode=hp.MATH_STRICT, cols=n, rows=rows, dx=dx)
    ref = oracle.OracleSim(n, rows, dx=dx)
    ref.upload(*gc.scene(real, n, rows))
    grids = gc.rates(0, 2, other, cells, real)
    for s in (dom, ref):
        s.add_gridded(hp.GRIDDED_RAIN_INTENSITY, grids, res, off, 0.0, 30.0)
    dom.set_target_time(1e9); ref.set_target(1e9)
    dom.step_batch(40); ref.run(40)                        # timesteps of 0.1 s at most in the first minute: the gate opens every ten or so
    got, want, sc, rsc = dom.download(), ref.download(), dom.read_scalars(), ref.scalars()
    dom.close()
    assert np.isfinite(want).all() and (want[1:-1, 1:-1, 0] > gc.scene(real, n, rows)[0][1:-1, 1:-1, 0]).mean() > 0.5     # it rained
    assert np.array_equal(got, want) and sc["time"] == rsc["t"] and sc["timestep"] == rsc["dt"] and rsc["t"] > 2.0


def test_two_strips_with_a_grid_line_in_the_ghost_rows_equal_the_single_domain():
    """Strips add row_offset to the row: 101 rows cut at row 50 (the strips store rows 0-50 and 49-100, one ghost row each), an uneven
    coarse grid whose row line lies between rows 49 and 50 -- each strip's ghost row belongs to another rain-grid row than the owned
    row next to it -- and whose column lines are off the window edges."""
    from test_gpu_strips import run_strips
    from hipims_mi import strips
    dx, res = 40.0, 66.7 * 40.0
    ox, oy = -0.37 * res, -16.95 * dx
    assert strips.partition(gc.ROWS, 2, 1) == [(0, 50, 0, 51), (50, 101, 49, 101)]
    row = gc.indices(np.float64, gc.ROWS, dx, oy, res)
    assert row[49] == 0 and row[50] == 1
    gr, gcols = gc.smallest_grid(np.float64, dx, res, ox, oy)
    rain = (gc.rates(0, gc.SLICES, gr, gcols, np.float64), res, ox, oy, gc.INTERVAL)
    st, bed, man = gc.scene(np.float64)
    steps = 25                                             # (before the first minute is over: 2 s, then 0.1 s a step -- rain at the second iteration and ten later)
    single = hp.Domain(gc.COLS, gc.ROWS, dx=dx, dt_initial=gc.DT0)
    single.upload(st, bed, man)
    single.add_gridded(hp.GRIDDED_RAIN_INTENSITY, *rain)
    assert single.boundaries_fused()
    single.set_target_time(1e9)
    single.step_batch(steps)
    want, sc = single.download(), single.read_scalars()
    single.close()
    ref = oracle.OracleSim(gc.COLS, gc.ROWS, dx=dx, dt_initial=gc.DT0)
    ref.upload(st, bed, man)
    ref.add_gridded(hp.GRIDDED_RAIN_INTENSITY, *rain)
    ref.set_target(1e9)
    ref.run(steps)
    depth = lambda s: np.maximum(0.0, s[..., 0] - bed)
    assert np.sqrt(np.mean((depth(want) - depth(ref.download())) ** 2)) < 1e-9 and (depth(want)[1:-1, 1:-1] > depth(st)[1:-1, 1:-1]).mean() > 0.5
    for overlap in (False, True):
        got, gsc = run_strips(gc.COLS, gc.ROWS, 2, hp.SCHEME_GODUNOV, steps, st, bed, man, rain=rain, overlap=overlap, dx=dx, dt_initial=gc.DT0)
        assert np.array_equal(got, want), overlap
        assert gsc["t"] == sc["time"] and gsc["dt"] == sc["timestep"]
