"""The selected cells of the output rasters as CSR, without a GPU: the NumPy restatement (frontend.sparse, combine_sparse,
sparse_to_dense -- the reference the GPU tests hold the device kernels to) on hand-made rasters, the entry point's argument checks
through the built library, the run planner of csrc/hp_sparse.hpp (sparse_plan_runs) in a stand-alone program, and the model file's
<sparseTarget> on the host path.  Selections and integer prefix sums only: there are no tolerances."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import hipims_mi as hp
import oracle
from conftest import ROOT
from hipims_mi import frontend
from model_dir import make_newcastle
from test_abi import HEADER, declared_functions

NODATA = -9999.0
CSRC = os.path.join(ROOT, "hipims-ocl_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))


def hand_made():
    """7 rows x 5 columns: row 0 empty, row 1 column 0 alone, row 2 the last column alone, a NaN and a -9999 in the select raster."""
    sel = np.array([[NODATA, NODATA, NODATA, NODATA, NODATA],
                    [0.5, NODATA, NODATA, NODATA, NODATA],
                    [NODATA, NODATA, NODATA, NODATA, 0.25],
                    [0.1, np.nan, 0.3, NODATA, 0.005],
                    [2.0, 2.5, 3.0, 3.5, 4.0],
                    [NODATA, 0.02, NODATA, 0.01, NODATA],
                    [-1.0, 0.0, -0.0, 1e-9, NODATA]])
    other = np.arange(35, dtype=np.float64).reshape(7, 5) - 17.0
    other[4, 2] = NODATA                              # a selected cell's other value may itself be NODATA
    return sel, other


def loop_sparse(rasters, sel, above):
    row_ptr, col, values = [0], [], [[] for _ in rasters]
    for y in range(sel.shape[0]):
        for x in range(sel.shape[1]):
            v = float(sel[y, x])
            if v != NODATA and v > above:
                col.append(x)
                for k, a in enumerate(rasters):
                    values[k].append(a[y, x])
        row_ptr.append(len(col))
    return row_ptr, col, values


def same_sparse(a, b):
    return (a[0].dtype == b[0].dtype == np.uint64 and a[1].dtype == b[1].dtype == np.uint32 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and len(a[2]) == len(b[2]) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a[2], b[2])))


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("above", [0.0, 0.01, 1e9, -np.inf, -1.0, 0.25])
def test_restatement_on_hand_made_rasters(above):
    sel, other = hand_made()
    row_ptr, col, (v_sel, v_other, v32) = frontend.sparse([sel, other, other.astype(np.float32)], sel, above)
    want = loop_sparse([sel, other], sel, above)
    assert row_ptr.dtype == np.uint64 and col.dtype == np.uint32 and v_sel.dtype == np.float64 and v32.dtype == np.float32
    assert row_ptr.tolist() == want[0] and col.tolist() == want[1]
    assert v_sel.tolist() == want[2][0] and v_other.tolist() == want[2][1] and np.array_equal(v32, v_other.astype(np.float32))
    assert not np.isnan(v_sel).any()                                              # a NaN fails the comparison
    if above == 0.0:
        assert row_ptr.tolist() == [0, 0, 1, 2, 5, 10, 12, 13] and col[:5].tolist() == [0, 4, 0, 2, 4]
        assert NODATA in v_other                                                   # delivered as it is
    if above == 1e9:
        assert row_ptr.tolist() == [0] * 8 and len(col) == 0 and len(v_sel) == 0
    if above == -np.inf:                                                           # everything that is neither NODATA nor a NaN
        assert len(col) == int(((sel != NODATA) & ~np.isnan(sel)).sum()) == 16
        every = frontend.sparse([other], other * 0.0 + 1.0, -np.inf)               # a value that is never NODATA: every cell
        assert every[0].tolist() == list(range(0, 36, 5)) and every[1].tolist() == list(range(5)) * 7 and np.array_equal(every[2][0], other.ravel())
    with pytest.raises(ValueError, match="NaN"):
        frontend.sparse([other], sel, np.nan)
    with pytest.raises(ValueError, match="shape"):
        frontend.sparse([other[:3]], sel, 0.0)


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_dense_again():
    sel, other = hand_made()
    for above in (0.0, 0.01, 1e9, -np.inf):
        row_ptr, col, (v_sel, v_other) = frontend.sparse([sel, other], sel, above)
        with np.errstate(invalid="ignore"):
            chosen = (sel != NODATA) & (sel > above)
        assert np.array_equal(frontend.sparse_to_dense(row_ptr, col, v_sel, 5), np.where(chosen, sel, NODATA))
        assert np.array_equal(frontend.sparse_to_dense(row_ptr, col, v_other, 5, fill=7.5), np.where(chosen, other, 7.5))
        dense32 = frontend.sparse_to_dense(row_ptr, col, v_other.astype(np.float32), 5)
        assert dense32.dtype == np.float32 and dense32.shape == (7, 5)


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_every_cut_of_a_seven_row_raster_combines_to_the_uncut_result():
    sel, other = hand_made()
    whole = frontend.sparse([sel, other], sel, 0.0)
    cuts = 0
    for mask in range(1 << 6):                                                     # a cut or none behind each of rows 0..5
        edges = [0] + [r + 1 for r in range(6) if mask >> r & 1] + [7]
        parts = [frontend.sparse([sel[lo:hi], other[lo:hi]], sel[lo:hi], 0.0) for lo, hi in zip(edges, edges[1:])]
        assert same_sparse(frontend.combine_sparse(parts), whole), edges
        cuts += 1
    assert cuts == 64
    empty = frontend.sparse([sel[:0], other[:0]], sel[:0], 0.0)                   # a part of no rows
    assert empty[0].tolist() == [0] and same_sparse(frontend.combine_sparse([empty, whole, empty]), whole)
    with pytest.raises(ValueError, match="no part"):
        frontend.combine_sparse([])


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    lib = hp.load_library()
    assert "hp_domain_sparse" in declared_functions() and hasattr(lib, "hp_domain_sparse") and "hp_domain_sparse" in hp.EXPORTS
    assert lib.hp_abi_version() == 2 and "#define HP_ABI_VERSION 2" in open(HEADER).read().replace("  ", " ")
    from hipims_mi import strips
    assert callable(hp.Domain.sparse) and callable(strips.StripRunner.gather_sparse) and callable(strips.HipEngine.sparse)
    # an older build has no such symbol: its signature is declared only where the symbol is, so the import does not raise
    assert 'if hasattr(lib, "hp_domain_sparse")' in inspect.getsource(hp.load_library)


def test_argument_errors_are_invalid_before_any_device_call():
    """With a NULL domain: every check that does not need the domain comes first and names what is wrong; the rest is "null
    domain".  No device is touched (this machine may have none)."""
    lib = hp.load_library()
    buf = np.zeros(64)
    cols = np.zeros(64, np.uint32)
    ints = lambda *v: (C.c_int * len(v))(*v)
    ptrs = lambda *v: (C.c_void_p * len(v))(*v)
    sel, rp = C.c_uint64(7), (C.c_uint64 * 4)(7, 7, 7, 7)
    col = cols.ctypes.data_as(C.POINTER(C.c_uint32))
    vals, ras = ints(hp.OUT_DEPTH, hp.OUT_FROUDE), ptrs(buf.ctypes.data, buf.ctypes.data)
    inf = float("inf")
    # (select_value, above, values, count, element_bytes, capacity, selected, row_ptr, col, rasters, row0, nrows)
    cases = [
        ((0, 0.0, vals, 2, 8, 8, None, rp, col, ras, 0, 0), "selected / row_ptr == NULL"),
        ((0, 0.0, vals, 2, 8, 8, C.byref(sel), None, col, ras, 0, 0), "selected / row_ptr == NULL"),
        ((0, 0.0, vals, 0, 8, 8, C.byref(sel), rp, col, ras, 0, 0), "count outside 1..HP_OUT_COUNT"),
        ((0, 0.0, vals, 10, 8, 8, C.byref(sel), rp, col, ras, 0, 0), "count outside 1..HP_OUT_COUNT"),
        ((0, 0.0, None, 2, 8, 8, C.byref(sel), rp, col, ras, 0, 0), "values == NULL"),
        ((0, 0.0, vals, 2, 2, 8, C.byref(sel), rp, col, ras, 0, 0), "element_bytes"),
        ((0, 0.0, vals, 2, 16, 8, C.byref(sel), rp, col, ras, 0, 0), "element_bytes"),
        ((9, 0.0, vals, 2, 8, 8, C.byref(sel), rp, col, ras, 0, 0), "unknown select_value 9"),
        ((-1, 0.0, vals, 2, 8, 8, C.byref(sel), rp, col, ras, 0, 0), "unknown select_value -1"),
        ((0, float("nan"), vals, 2, 8, 8, C.byref(sel), rp, col, ras, 0, 0), "above is a NaN"),
        ((0, 0.0, vals, 2, 8, 8, C.byref(sel), rp, None, ras, 0, 0), "capacity > 0 with col / rasters == NULL"),
        ((0, 0.0, vals, 2, 8, 8, C.byref(sel), rp, col, None, 0, 0), "capacity > 0 with col / rasters == NULL"),
        ((0, 0.0, vals, 2, 8, 8, C.byref(sel), rp, col, ptrs(buf.ctypes.data, None), 0, 0), "rasters[1] == NULL"),
        ((0, 0.0, ints(hp.OUT_DEPTH, hp.OUT_COUNT), 2, 8, 8, C.byref(sel), rp, col, ras, 0, 0), "unknown value 9"),
        ((0, 0.0, ints(-1, hp.OUT_FSL), 2, 8, 8, C.byref(sel), rp, col, ras, 0, 0), "unknown value -1"),
        ((0, 0.0, ints(hp.OUT_FSL, hp.OUT_FSL), 2, 8, 8, C.byref(sel), rp, col, ras, 0, 0), "value 2 listed twice"),
        ((0, 0.0, ints(hp.OUT_FSL, hp.OUT_FSL), 2, 8, 0, C.byref(sel), rp, None, None, 0, 0), "value 2 listed twice"),       # in a counting call too
        ((0, 0.0, vals, 2, 8, 8, C.byref(sel), rp, col, ras, 0, 0), "null domain"),
        ((hp.OUT_DISCHARGE_X, -inf, vals, 2, 4, 0, C.byref(sel), rp, None, None, 0, 0), "null domain"),                      # the counting call
        ((hp.OUT_FROUDE, inf, ints(*range(9)), 9, 8, 3, C.byref(sel), rp, col, ptrs(*[buf.ctypes.data] * 9), 0, 0), "null domain"),
    ]
    for args, message in cases:
        assert lib.hp_domain_sparse(None, *args) == -1, message
        assert message.encode() in lib.hp_last_error(), (message, lib.hp_last_error())
    assert sel.value == 7 and list(rp) == [7] * 4 and not cols.any() and not buf.any()      # a failing call writes nothing
    # (a row range outside the array and cols >= 2^32 need a domain, and a domain a device: tests/test_gpu_sparse.py)


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sparse") / "sparse_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "sparse_probe.cpp")])

    def run(cases):
        """[(bytes_per_entry, budget, row_ptr)] -> [[(row_lo, row_hi, first, count)]]"""
        text = "".join(" ".join(str(v) for v in [bpe, budget, len(rp) - 1] + list(rp)) + "\n" for bpe, budget, rp in cases)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(cases)
        return [[tuple(int(v) for v in run.split(":")) for run in line.split()] for line in out]
    return run


def test_the_planner_needs_no_hip():
    text = open(os.path.join(CSRC, "hp_sparse.hpp")).read()
    host = text.split("#ifdef __HIPCC__")[0]
    assert "sparse_plan_runs" in host and "hip" not in "\n".join(l.split("//")[0] for l in host.splitlines()).lower()


def test_runs_cover_the_entries_once_in_order_within_the_budget(planner):
    rng = np.random.default_rng(11)
    shapes = [[0, 3, 3, 10, 11, 11, 30, 31], [0, 0, 0, 0], [0, 5], [0, 0, 64, 64, 128, 1000, 1000, 1001, 1001], [0, 1, 2, 3, 4, 5]]
    shapes += [np.concatenate([[0], np.cumsum(rng.integers(0, 40, n) * (rng.random(n) < 0.7))]).tolist() for n in (1, 2, 17, 60)]
    cases = [(bpe, fit * bpe + slack, rp) for rp in shapes for bpe in (8, 12, 76) for fit in (1, 2, 3, 7, 64, 100, 10 ** 6) for slack in (0, bpe - 1)]
    got = planner(cases)
    split = False
    for (bpe, budget, rp), runs in zip(cases, got):
        fit, total, at = budget // bpe, rp[-1], 0
        for lo, hi, first, count in runs:
            assert first == at and count >= 1 and count * bpe <= budget and 0 <= lo < hi <= len(rp) - 1, (bpe, budget, rp, runs)
            assert rp[lo] <= first and first + count <= rp[hi], (rp, runs)      # the run's rows hold its entries
            if hi - lo > 1 or (first, count) == (rp[lo], rp[hi] - rp[lo]):        # whole rows ...
                assert first == rp[lo] and first + count == rp[hi]
            else:                                                                 # ... or a piece of ONE row larger than the budget
                assert hi == lo + 1 and rp[hi] - rp[lo] > fit
                split = True
            at += count
        assert at == total, (bpe, budget, rp, runs)
        if total <= fit and total:
            assert len(runs) == 1                                                 # what fits goes in one run
        for a, b in zip(runs, runs[1:]):                                          # greedy: the next run's first row would not have fitted
            if a[1] - a[0] >= 1 and a[2] == rp[a[0]] and a[2] + a[3] == rp[a[1]] and b[1] - b[0] >= 1 and b[2] == rp[b[0]]:
                nxt = next(r for r in range(a[1], len(rp) - 1) if rp[r + 1] > rp[r])
                assert rp[nxt + 1] - a[2] > fit, (rp, runs, fit)
    assert split
    # pinned by hand: budget of 10 entries
    assert planner([(8, 80, [0, 3, 3, 10, 11, 11, 30, 31])])[0] == [(0, 3, 0, 10), (3, 5, 10, 1), (5, 6, 11, 10), (5, 6, 21, 9), (6, 7, 30, 1)]
    assert planner([(8, 7, [0, 3]), (8, 800, [0, 0, 0])]) == [[], []]                # not one entry fits; nothing to cut


def test_the_planner_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Host code with its own main: built with the sanitizers and run on its own."""
    exe = tmp_path / "sparse_probe_san"
    r = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe),
                        os.path.join(HERE, "sparse_probe.cpp")], capture_output=True, text=True)
    if r.returncode != 0 and "asan" in r.stderr.lower() + r.stdout.lower():
        pytest.skip("this compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    text = "8 8 3 0 5 5 9\n76 760 4 0 0 100 100 101\n12 11 2 0 1 2\n4 4 0 0\n"
    res = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-2000:]
    assert res.stdout.split("\n")[:-1] == ["0:1:0:1 0:1:1:1 0:1:2:1 0:1:3:1 0:1:4:1 2:3:5:1 2:3:6:1 2:3:7:1 2:3:8:1",
                                           "1:2:0:10 1:2:10:10 1:2:20:10 1:2:30:10 1:2:40:10 1:2:50:10 1:2:60:10 1:2:70:10 1:2:80:10 1:2:90:10 3:4:100:1",
                                           "", ""]


# 6 ---------------------------------------------------------------------------------------------------------------------
def _oracle_sim(cfg, cols, rows, res):
    return oracle.OracleSim(cols, rows, dx=res, scheme=cfg.scheme, very_small=cfg.dry_threshold, courant=cfg.courant,
                            end_time=cfg.duration, friction=cfg.friction, threads=4)


def test_model_file_sparse_target_on_the_host_path(tmp_path):
    """<sparseTarget> parses, and a run writes one .npz per output time whose contents are frontend.sparse of the host derivation;
    the other targets are what they are without it.  (The oracle engine has no sparse(): this is the host path.)"""
    from hipims_mi.model import Model
    xml = make_newcastle(tmp_path / "s", duration=120, frequency=60)
    text = open(xml).read()
    marker = '<dataTarget type="raster" value="depth" format="HFA" target="depth_%t.img" />'
    assert marker in text
    open(xml, "w").write(text.replace(marker, marker + '\n<sparseTarget select="depth" above="0.01" values="depth,velocityX,velocityy" target="sparse_%t.npz"/>'))
    cfg = frontend.parse_configuration(xml)
    assert cfg.sparse == dict(select="depth", above=0.01, values=["depth", "velocityx", "velocityy"], target="sparse_%t.npz")
    assert [w for w, _ in cfg.targets] == ["depth", "velocityx", "velocityy", "fsl", "maxdepth"]       # the plain targets, as without it
    plain_xml = make_newcastle(tmp_path / "plain", duration=120, frequency=60)
    assert frontend.parse_configuration(plain_xml).sparse is None
    m = Model(xml, make_sim=_oracle_sim, output_format=".npy")
    plain = Model(plain_xml, make_sim=_oracle_sim, output_format=".npy")
    by_argument = Model(make_newcastle(tmp_path / "arg", duration=120, frequency=60), make_sim=_oracle_sim, output_format=".npy",
                        sparse=dict(select="froude", above=0.5, values=["froude", "maxdepth"], target="fast_%t"))
    assert not m.device_sparse and plain.sparse_spec is None and by_argument.sparse_spec["select"] == "froude"
    for model in (m, plain, by_argument):
        model.scheme.automatic_queue = False                                  # (batch boundaries are not physics-neutral: fixed)
        model.scheme.queue_addition_size = 16
    outs, plain_outs, arg_outs = m.run(), plain.run(), by_argument.run()
    state = m.sim.download()
    m.close(); plain.close(); by_argument.close()
    assert len(outs) == len(plain_outs) == len(arg_outs) == 2
    t, last = outs[-1]
    full = {v: frontend.derive_output(v, state, m.bed, m.res) for v in ("depth", "velocityx", "velocityy", "froude", "maxdepth")}
    want = frontend.sparse([full["depth"], full["velocityx"], full["velocityy"]], full["depth"], 0.01)
    got = last["sparse"]
    assert same_sparse((got["row_ptr"], got["col"], [got["depth"], got["velocityx"], got["velocityy"]]), want)
    assert 0 < len(want[1]) < full["depth"].size and (want[2][0] > 0.01).all()
    for time_, out in outs:
        f = np.load(os.path.join(str(tmp_path / "s"), "output", f"sparse_{int(time_)}.npz"))
        assert sorted(f.files) == sorted(["row_ptr", "col", "depth", "velocityx", "velocityy", "shape", "nodata", "select", "above"])
        assert f["shape"].tolist() == [195, 342] and f["nodata"] == NODATA and str(f["select"]) == "depth" and f["above"] == 0.01
        for key in ("row_ptr", "col", "depth", "velocityx", "velocityy"):
            assert f[key].dtype == out["sparse"][key].dtype and np.array_equal(f[key], out["sparse"][key]), key
        assert np.array_equal(frontend.sparse_to_dense(f["row_ptr"], f["col"], f["depth"], 342), np.where(out["depth"] > 0.01, out["depth"], NODATA))
    fast = np.load(os.path.join(str(tmp_path / "arg"), "output", f"fast_{int(t)}.npz"))
    want = frontend.sparse([full["froude"], full["maxdepth"]], full["froude"], 0.5)
    assert same_sparse((fast["row_ptr"], fast["col"], [fast["froude"], fast["maxdepth"]]), want) and str(fast["select"]) == "froude"
    # the other targets' files: byte for byte those of the run without the selection
    files = sorted(os.listdir(os.path.join(str(tmp_path / "plain"), "output")))
    assert len(files) == 10 and len(os.listdir(os.path.join(str(tmp_path / "s"), "output"))) == 12
    for f in files:
        assert open(os.path.join(str(tmp_path / "s"), "output", f), "rb").read() == open(os.path.join(str(tmp_path / "plain"), "output", f), "rb").read(), f
    for bad, message in ((dict(select="bed"), "unknown output"), (dict(values=["depth", "depth"]), "listed twice"), (dict(above=float("nan")), "NaN")):
        with pytest.raises(ValueError, match=message):
            Model(make_newcastle(tmp_path / "bad", duration=120, frequency=60), make_sim=_oracle_sim, output_format=None, sparse=bad)
