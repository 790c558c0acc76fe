"""The selected cells of the output rasters as CSR on the device (hp_domain_sparse; csrc/hp_sparse.hpp: sparse_select, sparse_scan_*,
sparse_scatter) against the NumPy restatement of the host derivation, frontend.sparse(frontend.derive_output(...)) on the
downloaded state -- bit for bit: between the predicate and the store everything is integers, so there are no tolerances, whatever
the launch shape.  The state is that of a short dam-break run over a bed with a wall row, a patch of disabled cells and land that
stays dry, so that every NODATA rule fires.  GPU only."""
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
SCAN_TILE = 1024                                        # csrc/hp_sparse.hpp: SPARSE_SCAN_TILE, segments per block of the scan
# lane-edge and wave-edge columns, a 3-column grid, several segments a row; and 2 x 1100 = 2200 segments: more than two blocks of the scan
GRIDS = [(67, 37), (130, 5), (3, 41), (517, 263), (65, 1100)]
SELECTIONS = [("depth", 0.0), ("depth", 0.01), ("depth", 1e9), ("dischargex", -np.inf), ("froude", 0.5)]
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

    def want(self, names, select, above, dtype=np.float64, row0=0, nrows=None):
        hi = self.dom.rows if nrows is None else row0 + nrows
        return frontend.sparse([self.full[n][row0:hi].astype(dtype) for n in names], self.full[select][row0:hi], above)


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


def same_sparse(a, b):
    return (a[0].dtype == b[0].dtype == np.uint64 and a[1].dtype == b[1].dtype == np.uint32 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and len(a[2]) == len(b[2]) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a[2], b[2])))


def assert_sparse(case, names, select, above, dtype=np.float64, row0=0, nrows=None):
    got = case.dom.sparse(names, select=select, above=above, dtype=dtype, row0=row0, nrows=nrows)
    want = case.want(names, select, above, dtype, row0, nrows)
    assert same_sparse(got, want), (names, select, above, dtype, row0, nrows, case.dom.cols, case.dom.rows, got[0][-1], want[0][-1])
    return got


def raw_call(dom, select, above, codes, element_bytes, capacity, row_ptr, col, arrays, row0, nrows):
    selected = C.c_uint64(2 ** 64 - 1)
    rc = dom.lib.hp_domain_sparse(dom.h, select, above, (C.c_int * len(codes))(*codes), len(codes), element_bytes, capacity, C.byref(selected),
                                  row_ptr.ctypes.data_as(C.POINTER(C.c_uint64)), None if col is None else col.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  None if arrays is None else (C.c_void_p * len(codes))(*[a.ctypes.data for a in arrays]), row0, nrows)
    return rc, selected.value


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("size", GRIDS)
def test_all_nine_values_and_each_one_alone_equal_the_restatement(cases, size, precision):
    case = cases(*size, precision)
    cols, rows = size
    if size == (65, 1100):
        assert rows * -(-cols // 64) > 2 * SCAN_TILE                                # the scan's block sums are scanned in turn
    for select, above in SELECTIONS:
        for dtype in (np.float64, np.float32):
            row_ptr, col, values = assert_sparse(case, NAMES, select, above, dtype)
            if above == 1e9:
                assert row_ptr[-1] == 0 and not row_ptr.any() and len(col) == 0
            if select == "dischargex":
                assert row_ptr[-1] == cols * rows and np.array_equal(col, np.tile(np.arange(cols, dtype=np.uint32), rows))
    for name in NAMES:
        assert_sparse(case, [name], "depth", 0.01)
        assert_sparse(case, [name], name, 0.0, np.float32)
    # the selected cells put back: the full raster where selected, NODATA elsewhere
    row_ptr, col, (depth,) = case.dom.sparse("depth", "depth", 0.01)
    assert np.array_equal(frontend.sparse_to_dense(row_ptr, col, depth, cols), np.where(case.full["depth"] > 0.01, case.full["depth"], NODATA))
    # every NODATA rule fires and water moves: the comparison above is not one of empty results
    if min(size) >= 9:
        depth = case.full["depth"]
        assert (depth == NODATA).any() and (depth > 0.5).any() and 0 < row_ptr[-1] < cols * rows
        assert (np.abs(case.state[..., 2]) > 1e-3).any() and (case.state[..., 1] == -9999.0).any() and (case.bed > 9999.0).any()
        assert (np.diff(row_ptr.astype(np.int64)) == 0).any()                      # the wall rows north and south: empty rows
        some = case.dom.sparse(["maxdepth"], "dischargex", -np.inf)                # a selected cell's other value may itself be NODATA: the walls
        assert (some[2][0] == NODATA).any() and (some[2][0] != NODATA).any()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("element_bytes", [8, 4])
def test_capacity(cases, element_bytes):
    """One entry short: row_ptr and selected are delivered and nothing else is written; the exact capacity delivers everything;
    capacity 0 with NULL col and rasters is the counting call."""
    case = cases(517, 263, "f64")
    dtype = np.float64 if element_bytes == 8 else np.float32
    codes = [hp.OUT_DEPTH, hp.OUT_VELOCITY_X, hp.OUT_MAXDEPTH]
    want = case.want(["depth", "velocityx", "maxdepth"], "depth", 0.01, dtype)
    total = int(want[0][-1])
    assert total > 1000
    row_ptr = np.full(264, 2 ** 64 - 1, np.uint64)
    rc, selected = raw_call(case.dom, hp.OUT_DEPTH, 0.01, codes, element_bytes, 0, row_ptr, None, None, 0, 263)
    assert (rc, selected) == (0, total) and np.array_equal(row_ptr, want[0])
    col = np.full(total + 8, 0xA5A5A5A5, np.uint32)
    arrays = [np.full(total + 8, -123.25, dtype) for _ in codes]
    row_ptr[:] = 2 ** 64 - 1
    rc, selected = raw_call(case.dom, hp.OUT_DEPTH, 0.01, codes, element_bytes, total - 1, row_ptr, col, arrays, 0, 263)
    case.dom.sync()
    assert (rc, selected) == (0, total) and np.array_equal(row_ptr, want[0])
    assert (col == 0xA5A5A5A5).all() and all((a == -123.25).all() for a in arrays)           # the canaries survive
    rc, selected = raw_call(case.dom, hp.OUT_DEPTH, 0.01, codes, element_bytes, total, row_ptr, col, arrays, 0, 263)
    case.dom.sync()
    assert (rc, selected) == (0, total)
    assert (col[total:] == 0xA5A5A5A5).all() and all((a[total:] == -123.25).all() for a in arrays)
    assert same_sparse((row_ptr, col[:total], [a[:total] for a in arrays]), want)
    # nothing selected: col untouched
    rc, selected = raw_call(case.dom, hp.OUT_DEPTH, 1e9, codes, element_bytes, total, row_ptr, col, arrays, 0, 263)
    case.dom.sync()
    assert (rc, selected) == (0, 0) and not row_ptr.any() and np.array_equal(col[:total], want[1])


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(67, 37), (517, 263)])
def test_row_ranges_combine_to_the_whole(cases, size):
    case = cases(*size, "f64")
    rows = size[1]
    names = ["depth", "velocityy", "froude"]
    whole = assert_sparse(case, names, "depth", 0.01)
    for edges in ([0, 1, rows], [0, rows // 2, rows // 2 + 1, rows], [0, 5, 17, rows - 1, rows]):          # each with a part one row high
        parts = [assert_sparse(case, names, "depth", 0.01, row0=lo, nrows=hi - lo) for lo, hi in zip(edges, edges[1:])]
        assert same_sparse(frontend.combine_sparse(parts), whole), edges
    for row0 in (0, 20, rows):                                                    # nrows == 0
        row_ptr, col, values = case.dom.sparse(names, "depth", 0.01, row0=row0, nrows=0)
        assert row_ptr.tolist() == [0] and len(col) == 0 and [len(v) for v in values] == [0, 0, 0]
    for row0, nrows in ((-1, 2), (0, rows + 1), (rows, 1), (rows + 1, 0), (3, -1)):
        with pytest.raises(hp.HipimsError, match=r"\(-1\).*out of bounds"):
            case.dom.sparse("depth", row0=row0, nrows=nrows)
    assert_sparse(case, names, "depth", 0.01)                                     # none of it has hurt the domain


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_entries_larger_than_the_scratch_cap_are_worked_through_in_runs_of_rows():
    """Nine fp64 values of every cell of 2100 x 1800: 76 B an entry is 287 MB, over the 256 MiB cap."""
    cols, rows = 2100, 1800
    assert 76 * cols * rows > 256 << 20
    case = Case(cols, rows, "f64", steps=4)
    try:
        got = assert_sparse(case, NAMES, "dischargex", -np.inf)
        assert got[0][-1] == cols * rows
        assert_sparse(case, ["depth", "froude"], "depth", 0.01, np.float32)
    finally:
        case.dom.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [hp.MATH_FAST, hp.MATH_STRICT])
def test_sparse_reads_between_batches_do_not_perturb_the_run(mode):
    cols, rows = 257, 130
    st, bed, man = dam_break(cols, rows, np.float64)
    seen = []
    for observed in (False, True):
        dom = hp.Domain(cols, rows, dx=DX, math_mode=mode)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        for k in range(8):
            dom.step_batch(8)
            if observed:
                dom.sparse(["depth", "froude", "velocityx"], ("depth", "froude", "dischargex")[k % 3], (0.01, 0.5, -np.inf)[k % 3], dtype=(np.float64, np.float32)[k % 2])
        ps = dom.pair_stats()
        seen.append((dom.download(), dom.read_scalars(), dom.launch_counts(), (ps["pairs"], ps["skipped_rows"], ps["still_rows"])))
        dom.close()
    plain, observed = seen
    assert np.array_equal(plain[0], observed[0])
    assert plain[1] == observed[1] and plain[1]["iterations"] == 64
    assert plain[2] == observed[2] and plain[3] == observed[3], (plain[2:], observed[2:])


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_inside_a_split_step_and_bad_arguments_on_a_live_domain(cases):
    case = cases(67, 37, "f64")
    dom, lib = case.dom, case.dom.lib
    want = case.want(["depth"], "depth", 0.01)
    total = int(want[0][-1])
    row_ptr, col, arrays = np.zeros(38, np.uint64), np.zeros(total, np.uint32), [np.zeros(total)]
    call = lambda row0, nrows: raw_call(dom, hp.OUT_DEPTH, 0.01, [hp.OUT_DEPTH], 8, total, row_ptr, col, arrays, row0, nrows)
    assert call(0, 38)[0] == -1 and b"out of bounds" in lib.hp_last_error()
    assert call(38, 0)[0] == -1 and b"out of bounds" in lib.hp_last_error()
    row_ptr[:] = 5
    assert call(37, 0) == (0, 0) and row_ptr[0] == 0 and (row_ptr[1:] == 5).all()      # nrows == 0 is HP_OK
    dom.step_begin()
    assert call(0, 37)[0] == -5
    assert b"hp_domain_sparse between hp_step_begin and hp_step_end" in lib.hp_last_error()
    dom.step_end()
    case.refresh()                                                               # (the step has changed the state)
    want = case.want(["depth"], "depth", 0.01)
    total = int(want[0][-1])
    col, arrays = np.zeros(total, np.uint32), [np.zeros(total)]
    assert call(0, 37) == (0, total)
    dom.sync()
    assert same_sparse((row_ptr, col, arrays), want)


# 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_strips_gather_sparse(world):
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", lib,
                               os.path.join(os.path.dirname(lib), "fake_rccl.cpp")])
    res = subprocess.run([sys.executable, os.path.join(HERE, "sparse_strips_worker.py"), str(world)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "sparse results identical in every word True" in res.stdout and "water selected True" in res.stdout


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_model_writes_the_sparse_target_from_the_device_as_from_the_host(tmp_path):
    from hipims_mi.model import Model
    from model_dir import make_newcastle
    marker = '<dataTarget type="raster" value="depth" format="HFA" target="depth_%t.img" />'
    extra = '\n<sparseTarget select="depth" above="0.01" values="depth,velocityx,velocityy" target="sparse_%t.npz"/>'
    runs = {}
    for tag, device in (("device", True), ("host", False)):
        xml = make_newcastle(tmp_path / tag, duration=240, frequency=120)
        text = open(xml).read()
        assert marker in text
        open(xml, "w").write(text.replace(marker, marker + extra))
        m = Model(xml, output_format=".npy", device_outputs=device)
        m.scheme.automatic_queue = False                                      # (batch boundaries are not physics-neutral: fixed)
        m.scheme.queue_addition_size = 64
        assert m.device_sparse is device
        runs[tag] = (m.run(), os.path.join(str(tmp_path / tag), "output"))
        m.close()
    (outs, out_dir), (host_outs, host_dir) = runs["device"], runs["host"]
    assert len(outs) == len(host_outs) == 2
    for (t, out), (_, host) in zip(outs, host_outs):
        a, b = np.load(os.path.join(out_dir, f"sparse_{int(t)}.npz")), np.load(os.path.join(host_dir, f"sparse_{int(t)}.npz"))
        assert sorted(a.files) == sorted(b.files) == sorted(["row_ptr", "col", "depth", "velocityx", "velocityy", "shape", "nodata", "select", "above"])
        for key in a.files:
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
        for key in ("row_ptr", "col", "depth", "velocityx", "velocityy"):
            assert np.array_equal(out["sparse"][key], a[key]) and np.array_equal(host["sparse"][key], a[key])
        assert np.array_equal(frontend.sparse_to_dense(a["row_ptr"], a["col"], a["depth"], 342), np.where(out["depth"] > 0.01, out["depth"], NODATA))
    assert 0 < len(np.load(os.path.join(out_dir, f"sparse_{int(outs[-1][0])}.npz"))["col"]) < 195 * 342
