"""Block-aggregated overviews on the device (hp_domain_overview; csrc/hp_overview.hpp: overview_blocks, overview_finish) against
the NumPy restatement of the host derivation, frontend.overview(frontend.derive_output(...)) on the downloaded state -- bit for
bit: what the kernel accumulates is integers, so there are no tolerances, whatever the launch shape or the order in which the
atomics arrive.  The state is that of a short dam-break run over a bed with a wall row, a patch of disabled cells and land that
stays dry, so that every NODATA rule fires.  The library refuses grids narrower than three columns: the "single column" is a
3-column grid, one column of blocks for every factor from 3 on.  GPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hipims_mi as hp
from hipims_mi import frontend

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["depth", "maxdepth", "fsl", "maxfsl", "dischargex", "dischargey", "velocityx", "velocityy", "froude"]
KINDS = ("max", "min", "count")
PAIRS = [(name, kind) for name in NAMES for kind in KINDS]                     # all 27
FACTORS = (1, 2, 3, 16, 64, 100, 4096)
GRIDS = [(67, 37), (130, 5), (3, 41), (517, 263)]       # lane-edge and wave-edge columns, one column of blocks, several workgroups a row
DX = 2.5
NODATA = frontend.NODATA


def dam_break(cols, rows, real):
    """Moving water of level 1.6 m behind x = 0.4 cols over an undulating bed that rises to the east (the land there stays dry), a ring of
    closed-edge walls, a wall row across two thirds of the grid and a patch of disabled cells."""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    bed = np.round((0.3 * np.sin(x / 5.0) * np.cos(y / 3.0) + 2.5 * x / max(cols - 1, 1)) * 1e4) / 1e4
    st = np.zeros((rows, cols, 4))
    st[..., 0] = st[..., 1] = np.maximum(bed, np.where(x < 0.4 * cols, 1.6, 0.3))
    wet = st[..., 0] - bed > 0.1
    st[..., 2] = np.where(wet, np.round(0.2 * np.sin(y + 0.5) * 1e4) / 1e4, 0.0)          # water that moves both ways
    st[..., 3] = np.where(wet, np.round(0.2 * np.cos(x + 0.5) * 1e4) / 1e4, 0.0)
    for sl in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        bed[sl] = 9999.9
        st[sl] = 0.0
    if rows >= 9:
        wall = np.s_[rows // 2, :max(2, 2 * cols // 3)]
        bed[wall] = 9999.9
        st[wall] = 0.0
    if rows >= 9 and cols >= 9:
        st[2:5, 3:6, 1] = -9999.0                                             # disabled: Zmax = -9999
    return st.astype(real), bed.astype(real), np.full((rows, cols), 0.03, real)


class Case:
    """A developed domain, its downloaded state and the nine full rasters of the host derivation (computed once)."""

    def __init__(self, cols, rows, precision, steps=12, **kw):
        real = np.float64 if precision == "f64" else np.float32
        st, self.bed, man = dam_break(cols, rows, real)
        self.dom = hp.Domain(cols, rows, dx=DX, precision=precision, **kw)
        self.dom.upload(st, self.bed, man)
        self.dom.set_target_time(1e9)
        self.dom.step_batch(steps)
        self.refresh()

    def refresh(self):
        self.state = self.dom.download()
        self.full = {name: frontend.derive_output(name, self.state, self.bed, DX) for name in NAMES}

    def want(self, name, kind, factor, row0=0, nrows=None, row_offset=0):
        hi = self.dom.rows if nrows is None else row0 + nrows
        return frontend.overview(self.full[name][row0:hi], factor, kind, row_offset + row0)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(cols, rows, precision):
        if (cols, rows, precision) not in made:
            made[(cols, rows, precision)] = Case(cols, rows, precision)
        return made[(cols, rows, precision)]
    yield get
    for c in made.values():
        c.dom.close()


def same_bits(got, want):
    u = np.uint64 if want.dtype == np.float64 else np.uint32
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(u), want.view(u))


def assert_overviews(case, factor, dtype=np.float64, row0=0, nrows=None, pairs=PAIRS):
    got = case.dom.overview([n for n, _ in pairs], [k for _, k in pairs], factor, dtype=dtype, row0=row0, nrows=nrows)
    assert len(got) == len(pairs)
    for (name, kind), g in zip(pairs, got):
        want = case.want(name, kind, factor, row0, nrows).astype(dtype)          # (fp32: rounded once, after the aggregation)
        assert same_bits(g, want), (name, kind, factor, row0, nrows, case.dom.cols, case.dom.rows, int((g != want).sum()), g.shape, want.shape)
    return got


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("size", GRIDS)
def test_all_27_pairs_in_one_call_equal_the_restatement(cases, size, precision):
    case = cases(*size, precision)
    rows, cols = case.bed.shape
    for factor in FACTORS:
        got = assert_overviews(case, factor)
        assert_overviews(case, factor, dtype=np.float32)
        assert case.dom.overview_shape(factor) == hp.overview_shape(cols, factor, 0, 0, rows) == (0, got[0].shape[0], got[0].shape[1])
    # factor 1: the largest and the smallest of a cell alone are hp_domain_derive's raster
    full = case.dom.derive(NAMES)
    one = case.dom.overview(NAMES + NAMES, ["max"] * 9 + ["min"] * 9, 1)
    for k, name in enumerate(NAMES):
        assert not np.isnan(full[name]).any()
        assert same_bits(one[k], full[name]) and same_bits(one[9 + k], full[name]), name
    # every NODATA rule fires and water moves: the comparison above is not one of empty rasters
    if min(size) >= 9:
        depth = case.full["depth"]
        assert (depth == NODATA).any() and (depth > 0.5).any() and (case.full["velocityx"] != NODATA).any()
        assert (np.abs(case.state[..., 2]) > 1e-3).any() and (case.state[..., 1] == -9999.0).any() and (case.bed > 9999.0).any()
        assert (case.full["velocityx"][case.full["velocityx"] != NODATA] < 0).any()          # signed values


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_a_block_without_a_participating_cell(cases):
    """The land in the east stays dry: whole blocks of NODATA depth, and a count of 0 there."""
    case = cases(517, 263, "f64")
    mx, mn, n = case.dom.overview(["depth"] * 3, KINDS, 16)
    empty = n == 0
    assert empty.any() and not empty.all()
    assert (mx[empty] == NODATA).all() and (mn[empty] == NODATA).all() and (mx[~empty] > 0).all() and (mn[~empty] > 0).all()
    assert n.sum() == (case.full["depth"] != NODATA).sum() and n.max() <= 256 and (mn[~empty] <= mx[~empty]).all()
    n32 = case.dom.overview("depth", "count", 4096, dtype=np.float32)[0]
    assert n32.dtype == np.float32 and n32.shape == (1, 1) and n32[0, 0] == n.sum()


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(67, 37), (517, 263)])
def test_row_ranges_that_start_and_end_inside_a_block(cases, size):
    case = cases(*size, "f64")
    rows = size[1]
    pairs = [("depth", "max"), ("velocityx", "min"), ("froude", "count"), ("fsl", "min")]
    for row0, nrows in ((5, 17), (1, 1), (rows - 1, 1), (10, 20), (0, 16), (16, 16), (15, 2), (7, rows - 7)):
        for factor in (16, 3, 100):
            got = assert_overviews(case, factor, row0=row0, nrows=nrows, pairs=pairs)
            first, brows, bcols = case.dom.overview_shape(factor, row0, nrows)
            assert (first, brows, bcols) == hp.overview_shape(size[0], factor, 0, row0, nrows) and got[0].shape == (brows, bcols)
    for row0 in (0, 20, rows):
        empty = case.dom.overview(["depth", "froude"], ["max", "count"], 16, row0=row0, nrows=0)
        assert [e.shape for e in empty] == [(0, -(-size[0] // 16))] * 2
    for row0, nrows in ((-1, 2), (0, rows + 1), (rows, 1), (rows + 1, 0), (3, -1)):
        with pytest.raises(hp.HipimsError, match=r"\(-1\).*out of bounds"):
            case.dom.overview("depth", "max", 16, row0=row0, nrows=nrows)
    for factor in (0, 4097):
        with pytest.raises(hp.HipimsError, match=r"\(-1\).*factor outside"):
            case.dom.overview("depth", "max", factor)
    assert_overviews(case, 16, pairs=pairs)                                       # none of it has hurt the domain


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("size", [(67, 37), (517, 263)])
def test_the_result_does_not_depend_on_the_cut(cases, size, dtype):
    """One call, and two calls split at a row that is no multiple of the factor, put together by combine_overviews."""
    case = cases(*size, "f64")
    rows = size[1]
    for factor in (16, 3, 64):
        cuts = [c for c in (factor + 1, rows // 2 + 1, rows // 2 + 2, rows - 1, rows - 2) if c % factor and 0 < c < rows][:3]
        assert len(cuts) == 3
        for cut in cuts:
            whole = case.dom.overview([n for n, _ in PAIRS], [k for _, k in PAIRS], factor, dtype=dtype)
            south = case.dom.overview([n for n, _ in PAIRS], [k for _, k in PAIRS], factor, dtype=dtype, row0=0, nrows=cut)
            north = case.dom.overview([n for n, _ in PAIRS], [k for _, k in PAIRS], factor, dtype=dtype, row0=cut, nrows=rows - cut)
            firsts = (case.dom.overview_shape(factor, 0, cut)[0], case.dom.overview_shape(factor, cut, rows - cut)[0])
            assert firsts == (0, cut // factor)
            for k, (name, kind) in enumerate(PAIRS):
                first, got = frontend.combine_overviews([(firsts[1], north[k]), (firsts[0], south[k])], kind)
                assert first == 0 and same_bits(got, whole[k]), (name, kind, factor, cut)


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_a_request_larger_than_the_scratch_cap_is_worked_through_in_runs_of_block_rows():
    """27 pairs at factor 1 on 1000 x 700 cells: 27 x 16 B per block is 302 MB of accumulators and elements, over the 256 MiB cap."""
    cols, rows = 1000, 700
    assert 27 * 16 * cols * rows > 256 << 20
    case = Case(cols, rows, "f64", steps=6)
    try:
        assert_overviews(case, 1)
        assert_overviews(case, 7, pairs=PAIRS[::4])
    finally:
        case.dom.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [hp.MATH_FAST, hp.MATH_STRICT])
def test_overviews_between_batches_do_not_perturb_the_run(mode):
    cols, rows = 257, 130
    real = np.float64
    st, bed, man = dam_break(cols, rows, real)
    seen = []
    for observed in (False, True):
        dom = hp.Domain(cols, rows, dx=DX, math_mode=mode)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        for k in range(8):
            dom.step_batch(8)
            if observed:
                dom.overview(["depth", "froude", "velocityx"], ["max", "max", "min"], (4, 16, 100)[k % 3], dtype=(np.float64, np.float32)[k % 2])
        ps = dom.pair_stats()
        seen.append((dom.download(), dom.read_scalars(), dom.launch_counts(), (ps["pairs"], ps["skipped_rows"], ps["still_rows"])))
        dom.close()
    plain, observed = seen
    assert np.array_equal(plain[0], observed[0])
    assert plain[1] == observed[1] and plain[1]["iterations"] == 64
    assert plain[2] == observed[2] and plain[3] == observed[3], (plain[2:], observed[2:])


# 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("size", GRIDS)
def test_derive_is_what_the_host_derivation_gives(cases, size, precision):
    """hp_domain_derive shares the per-cell value with the overview kernel now: its rasters are still the host derivation's."""
    case = cases(*size, precision)
    for dtype in (np.float64, np.float32):
        got = case.dom.derive(NAMES, dtype=dtype)
        for name in NAMES:
            assert same_bits(got[name], case.full[name].astype(dtype)), (name, dtype)
    part = case.dom.derive(["velocityy", "maxdepth"], row0=1, nrows=size[1] - 2)
    assert same_bits(part["velocityy"], case.full["velocityy"][1:-1]) and same_bits(part["maxdepth"], case.full["maxdepth"][1:-1])


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_inside_a_split_step_and_bad_arguments_on_a_live_domain(cases):
    case = cases(67, 37, "f64")
    dom, lib = case.dom, case.dom.lib
    buf = np.zeros((3, 5))
    vals, aggs, ras = (C.c_int * 1)(hp.OUT_DEPTH), (C.c_int * 1)(hp.AGG_MAX), (C.c_void_p * 1)(buf.ctypes.data)
    assert lib.hp_domain_overview(dom.h, vals, aggs, 1, 16, 8, ras, 0, 38) == -1 and b"out of bounds" in lib.hp_last_error()
    assert lib.hp_domain_overview(dom.h, vals, aggs, 1, 16, 3, ras, 0, 37) == -1 and b"element_bytes" in lib.hp_last_error()
    assert lib.hp_domain_overview(dom.h, vals, (C.c_int * 1)(3), 1, 16, 8, ras, 0, 37) == -1 and b"unknown aggregate 3" in lib.hp_last_error()
    assert lib.hp_domain_overview(dom.h, vals, aggs, 1, 16, 8, ras, 37, 0) == 0                       # nrows == 0 is HP_OK
    dom.step_begin()
    assert lib.hp_domain_overview(dom.h, vals, aggs, 1, 16, 8, ras, 0, 37) == -5
    assert b"hp_domain_overview between hp_step_begin and hp_step_end" in lib.hp_last_error()
    dom.step_end()
    case.refresh()                                                               # (the step has changed the state)
    assert lib.hp_domain_overview(dom.h, vals, aggs, 1, 16, 8, ras, 0, 37) == 0
    dom.sync()
    assert same_bits(buf, case.want("depth", "max", 16))
    assert_overviews(case, 3)


# 9 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_strips_gather_overview(world):
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", lib,
                               os.path.join(os.path.dirname(lib), "fake_rccl.cpp")])
    res = subprocess.run([sys.executable, os.path.join(HERE, "overview_strips_worker.py"), str(world)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "overviews identical in every bit True" in res.stdout and "water in the picture True" in res.stdout


# 10 --------------------------------------------------------------------------------------------------------------------
def test_model_writes_an_overview_target_from_the_device(tmp_path):
    from hipims_mi.model import Model
    from model_dir import make_newcastle
    marker = '<dataTarget type="raster" value="depth" format="HFA" target="depth_%t.img" />'
    extra = ('\n<dataTarget type="raster" value="depth" overview="4" target="depth4_%t.img" />'
             '\n<dataTarget type="raster" value="froude" overview="16" aggregate="count" target="wet16_%t.img" />')
    runs = {}
    for tag in ("with", "without"):
        xml = make_newcastle(tmp_path / tag, duration=240, frequency=120)
        text = open(xml).read()
        assert marker in text
        if tag == "with":
            open(xml, "w").write(text.replace(marker, marker + extra))
        m = Model(xml, output_format=".npy")
        m.scheme.automatic_queue = False                                      # (batch boundaries are not physics-neutral: fixed)
        m.scheme.queue_addition_size = 64
        assert m.device_outputs and m.device_overviews is (tag == "with")
        outs = m.run()
        runs[tag] = (outs, os.path.join(str(tmp_path / tag), "output"), m.res)
        m.close()
    outs, out_dir, res = runs["with"]
    assert len(outs) == 2
    for t, out in outs:
        assert same_bits(out[("depth", "max", 4)], frontend.overview(out["depth"], 4, "max"))     # depth is a plain target too: its full raster
        for key, name in ((("depth", "max", 4), "depth4"), (("froude", "count", 16), "wet16")):
            assert np.array_equal(np.load(os.path.join(out_dir, f"{name}_{int(t)}.npy")), out[key])
        assert out[("depth", "max", 4)].shape == (49, 86) and out[("froude", "count", 16)].shape == (13, 22)
    assert (outs[-1][1][("depth", "max", 4)] > 0).any() and outs[-1][1][("froude", "count", 16)].sum() > 0
    # the count of cells with a Froude number is the count of cells with a velocity, whose full raster the run wrote as well
    t, out = outs[-1]
    assert same_bits(out[("froude", "count", 16)], frontend.overview(out["velocityx"], 16, "count"))
    plain = sorted(os.listdir(runs["without"][1]))
    assert len(plain) == 10 and len(os.listdir(out_dir)) == 14
    for f in plain:
        assert open(os.path.join(out_dir, f), "rb").read() == open(os.path.join(runs["without"][1], f), "rb").read(), f
