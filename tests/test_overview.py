"""Block-aggregated overviews without a GPU: the two entry points and their argument checks, the block arithmetic
(hipims_mi.overview_shape, the restatement of hp_overview_shape), the NumPy restatement (frontend.overview, the reference the GPU
tests hold the device kernel to) against a plain Python loop, its independence of the cut of a row range
(frontend.combine_overviews), and the model file's `overview` attribute on the host path.  Maxima, minima and counts only: there
are no tolerances."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import hipims_mi as hp
import oracle
from hipims_mi import frontend
from model_dir import make_newcastle
from test_abi import HEADER, declared_functions

NODATA = -9999.0
KINDS = ("max", "min", "count")


def loop_overview(a, factor, kind, row_offset=0):
    """One overview in plain Python: three loops, floats compared as floats."""
    rows, cols = a.shape
    first = row_offset // factor
    brows, bcols = (row_offset + rows - 1) // factor - first + 1, -(-cols // factor)
    out = [[None] * bcols for _ in range(brows)]
    for by in range(brows):
        for bx in range(bcols):
            seen = []
            for y in range(rows):
                for x in range(cols):
                    v = float(a[y, x])
                    if (row_offset + y) // factor - first == by and x // factor == bx and v != NODATA and not math.isnan(v):
                        seen.append(v)
            out[by][bx] = float(len(seen)) if kind == "count" else (NODATA if not seen else (max(seen) if kind == "max" else min(seen)))
    return np.array(out, np.float64)


def hand_made(rows=7, cols=5, seed=3):
    """Signed values with NODATA cells, NaN cells, a column of nothing but NODATA and a row of nothing but NaN."""
    a = np.random.default_rng(seed).normal(0.0, 3.0, (rows, cols))
    a[1, 1] = a[4, 0] = a[6, 4] = NODATA
    a[2, 3] = a[5, 2] = np.nan
    a[:, cols - 1] = NODATA
    a[0, :] = np.nan
    return a


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    lib = hp.load_library()
    for n in ("hp_overview_shape", "hp_domain_overview"):
        assert n in declared_functions() and hasattr(lib, n) and n in hp.EXPORTS
    header = open(HEADER).read()
    assert "enum { HP_AGG_MAX = 0, HP_AGG_MIN = 1, HP_AGG_COUNT = 2, HP_AGG_KINDS = 3 };" in header
    assert (hp.AGG_MAX, hp.AGG_MIN, hp.AGG_COUNT, hp.AGG_KINDS) == (0, 1, 2, 3)
    assert hp.AGG_CODES == {"max": 0, "min": 1, "count": 2} and frontend.AGGREGATES == KINDS


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_invalid_before_any_device_call():
    """With a NULL domain: every check that does not need the domain comes first and names what is wrong; the rest is "null
    domain".  No device is touched (this machine may have none)."""
    lib = hp.load_library()
    buf = np.zeros(64)
    ints = lambda *v: (C.c_int * len(v))(*v)
    ptrs = lambda *v: (C.c_void_p * len(v))(*v)
    vals, aggs, ras = ints(hp.OUT_DEPTH, hp.OUT_FROUDE), ints(hp.AGG_MAX, hp.AGG_COUNT), ptrs(buf.ctypes.data, buf.ctypes.data)
    every = [(v, a) for v in range(9) for a in range(3)]
    cases = [
        ((vals, aggs, 0, 4, 8, ras, 0, 0), "count outside 1..27"),
        ((vals, aggs, 28, 4, 8, ras, 0, 0), "count outside 1..27"),
        ((None, aggs, 2, 4, 8, ras, 0, 0), "== NULL"),
        ((vals, None, 2, 4, 8, ras, 0, 0), "== NULL"),
        ((vals, aggs, 2, 4, 8, None, 0, 0), "== NULL"),
        ((vals, aggs, 2, 4, 2, ras, 0, 0), "element_bytes"),
        ((vals, aggs, 2, 4, 16, ras, 0, 0), "element_bytes"),
        ((vals, aggs, 2, 0, 8, ras, 0, 0), "factor outside 1..4096"),
        ((vals, aggs, 2, -3, 8, ras, 0, 0), "factor outside 1..4096"),
        ((vals, aggs, 2, 4097, 8, ras, 0, 0), "factor outside 1..4096"),
        ((ints(hp.OUT_DEPTH, hp.OUT_COUNT), aggs, 2, 4, 8, ras, 0, 0), "unknown value 9"),
        ((ints(-1, hp.OUT_FSL), aggs, 2, 4, 8, ras, 0, 0), "unknown value -1"),
        ((vals, ints(hp.AGG_MAX, hp.AGG_KINDS), 2, 4, 8, ras, 0, 0), "unknown aggregate 3"),
        ((vals, ints(-1, hp.AGG_MIN), 2, 4, 8, ras, 0, 0), "unknown aggregate -1"),
        ((ints(hp.OUT_FSL, hp.OUT_FSL), ints(hp.AGG_MIN, hp.AGG_MIN), 2, 4, 8, ras, 0, 0), "pair (2, 1) listed twice"),
        ((vals, aggs, 2, 4, 8, ptrs(buf.ctypes.data, None), 0, 0), "rasters[1] == NULL"),
        ((vals, aggs, 2, 4, 8, ras, 0, 0), "null domain"),
        ((ints(hp.OUT_FSL, hp.OUT_FSL), ints(hp.AGG_MIN, hp.AGG_MAX), 2, 4096, 4, ras, 0, 0), "null domain"),      # one value, two aggregates
        ((ints(*[v for v, _ in every]), ints(*[a for _, a in every]), 27, 1, 8, ptrs(*[buf.ctypes.data] * 27), 0, 0), "null domain"),
    ]
    for args, message in cases:
        assert lib.hp_domain_overview(None, *args) == -1, message
        assert message.encode() in lib.hp_last_error(), (message, lib.hp_last_error())
    a, b, c = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    for args, message in [((0, 0, 0, C.byref(a), C.byref(b), C.byref(c)), "factor outside 1..4096"),
                          ((4097, 0, 0, C.byref(a), C.byref(b), C.byref(c)), "factor outside 1..4096"),
                          ((4, 0, 0, None, C.byref(b), C.byref(c)), "== NULL"),
                          ((4, 0, 0, C.byref(a), None, C.byref(c)), "== NULL"),
                          ((4, 0, 0, C.byref(a), C.byref(b), None), "== NULL"),
                          ((4, 0, 0, C.byref(a), C.byref(b), C.byref(c)), "null domain")]:
        assert lib.hp_overview_shape(None, *args) == -1, message
        assert message.encode() in lib.hp_last_error(), (message, lib.hp_last_error())
    assert (a.value, b.value, c.value) == (7, 7, 7)                                # a failing call writes nothing


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_block_arithmetic():
    """hp_overview_shape needs a domain, and a domain a device: the formula is pinned through the module's restatement (the GPU
    suite holds the library's answers to it).  -> (first_block_row, block_rows, block_cols)"""
    shape = hp.overview_shape
    assert shape(67, 16, 0, 0, 37) == (0, 3, 5)                                     # a partial last block in both directions
    assert shape(64, 16, 0, 0, 32) == (0, 2, 4)
    assert shape(67, 100, 0, 0, 37) == (0, 1, 1)                                    # a factor above the grid
    assert shape(67, 4096, 0, 0, 37) == (0, 1, 1)
    assert shape(1, 1, 0, 0, 9) == (0, 9, 1)
    # row_offset != 0: blocks are anchored to the global grid
    assert shape(130, 16, row_offset=40, row0=0, nrows=20) == (2, 2, 9)              # global rows 40..59: block rows 2 and 3
    assert shape(130, 16, row_offset=40, row0=8, nrows=8) == (3, 1, 9)               # 48..55: block row 3 alone
    assert shape(130, 16, row_offset=40, row0=7, nrows=18) == (2, 3, 9)              # 47..64: starts and ends inside a block
    assert shape(130, 3, row_offset=43, row0=1, nrows=1) == (14, 1, 44)
    assert shape(130, 100, row_offset=250, row0=0, nrows=60) == (2, 2, 2)            # 250..309 with a factor above the strip height
    assert shape(130, 16, row_offset=40, row0=5, nrows=0) == (2, 0, 9)               # nothing asked for
    for cols, factor, off, row0, nrows in [(67, 3, 5, 2, 31), (5, 7, 1000, 3, 4), (4097, 4096, 4095, 0, 2)]:
        first, brows, bcols = shape(cols, factor, off, row0, nrows)
        touched = sorted({(off + row0 + r) // factor for r in range(nrows)})
        assert (first, brows) == (touched[0], len(touched)) and touched == list(range(first, first + brows))
        assert bcols == len({x // factor for x in range(cols)})
    for bad in (0, 4097, -1):
        with pytest.raises(ValueError, match="factor"):
            shape(10, bad, 0, 0, 1)
    with pytest.raises(ValueError, match="row range"):
        shape(10, 2, 0, 0, -1)


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_against_a_plain_loop(kind):
    a = hand_made()
    assert a.shape == (7, 5)
    for factor in (1, 2, 3, 5, 7, 100, 4096):
        for row_offset in (0, 1, 2, 9):
            got = frontend.overview(a, factor, kind, row_offset)
            want = loop_overview(a, factor, kind, row_offset)
            assert got.dtype == np.float64 and got.shape == want.shape, (factor, row_offset)
            assert np.array_equal(got, want), (factor, row_offset, got, want)
            assert np.array_equal(frontend.overview(a, factor, hp.AGG_CODES[kind], row_offset), got)       # by code
    # the column of NODATA and the row of NaN take part nowhere
    one = frontend.overview(a, 1, kind)
    empty = 0.0 if kind == "count" else NODATA
    assert (one[:, 4] == empty).all() and (one[0, :] == empty).all() and not np.isnan(one).any()
    if kind != "count":                                                                # factor 1 is the raster itself, NaN -> NODATA
        assert np.array_equal(one, np.where(np.isnan(a), NODATA, a))
    # an fp32 domain's values, widened; and the signed zeros: -0.0 lies below +0.0
    a32 = a.astype(np.float32)
    assert np.array_equal(frontend.overview(a32, 3, kind, 1), loop_overview(a32.astype(np.float64), 3, kind, 1))
    zeros = np.array([[0.0, -0.0], [-0.0, 0.0]])
    assert bool(np.signbit(frontend.overview(zeros, 2, "min")[0, 0])) and not np.signbit(frontend.overview(zeros, 2, "max")[0, 0])
    with pytest.raises(ValueError, match="unknown aggregate"):
        frontend.overview(a, 2, "sum")
    with pytest.raises(ValueError, match="factor"):
        frontend.overview(a, 0, kind)


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cuts", [(4,), (9,), (16,), (5, 11), (1, 2), (16, 32)])
def test_combined_parts_equal_the_uncut_overview(cuts, kind):
    """Two and three row cuts, in the middle of a block (factor 16: rows 4, 9, 5, 11, 1, 2 with the offset 3) and on a block
    border; float64 parts and parts rounded to float32."""
    rows, cols, off = 37, 67, 3
    rng = np.random.default_rng(sum(cuts))
    a = rng.normal(0.0, 2.0, (rows, cols))
    a[rng.random((rows, cols)) < 0.4] = NODATA
    a[5:35, 10:50] = NODATA                                                            # blocks in which nothing takes part
    a[3, 3] = np.nan
    edges = (0,) + cuts + (rows,)
    for factor in (16, 3, 100):
        whole = frontend.overview(a, factor, kind, off)
        parts = [(hp.overview_shape(cols, factor, off, lo, hi - lo)[0], frontend.overview(a[lo:hi], factor, kind, off + lo))
                 for lo, hi in zip(edges, edges[1:])]
        first, got = frontend.combine_overviews([None] + parts[::-1], kind)            # any order; None entries are skipped
        assert first == off // factor and got.dtype == np.float64 and got.shape == whole.shape
        assert np.array_equal(got.view(np.uint64), whole.view(np.uint64)), (factor, cuts)
        first32, got32 = frontend.combine_overviews([(f, p.astype(np.float32)) for f, p in parts], kind)
        assert first32 == first and got32.dtype == np.float32 and np.array_equal(got32.view(np.uint32), whole.astype(np.float32).view(np.uint32))
        if kind == "count":
            assert got.sum() == ((a != NODATA) & ~np.isnan(a)).sum()
        else:
            assert (got == NODATA).any() or factor == 100
    with pytest.raises(ValueError, match="no part"):
        frontend.combine_overviews([None], kind)
    with pytest.raises(ValueError, match="differ"):
        frontend.combine_overviews([(0, np.zeros((1, 2))), (1, np.zeros((1, 3)))], kind)


# 6 ---------------------------------------------------------------------------------------------------------------------
def _oracle_sim(cfg, cols, rows, res):
    return oracle.OracleSim(cols, rows, dx=res, scheme=cfg.scheme, very_small=cfg.dry_threshold, courant=cfg.courant,
                            end_time=cfg.duration, friction=cfg.friction, threads=4)


def test_model_file_overview_targets_on_the_host_path(tmp_path):
    """A <dataTarget overview="4"> is written as the restatement of the full raster, with resolution factor * dx; the other targets
    are what they are without it.  (The oracle engine has no overview(): this is the host path.)"""
    from hipims_mi.model import Model
    xml = make_newcastle(tmp_path / "o", duration=120, frequency=60)
    text = open(xml).read()
    marker = '<dataTarget type="raster" value="depth" format="HFA" target="depth_%t.img" />'
    assert marker in text
    open(xml, "w").write(text.replace(marker, marker + '\n<dataTarget type="raster" value="depth" overview="4" target="depth4_%t.img" />'
                                      '\n<dataTarget type="raster" value="velocityX" overview="16" aggregate="MIN" target="velx16_%t.img" />'))
    cfg = frontend.parse_configuration(xml)
    assert cfg.overviews == [("depth", "max", 4, "depth4_%t.img", ""), ("velocityx", "min", 16, "velx16_%t.img", "")]
    assert [w for w, _ in cfg.targets] == ["depth", "velocityx", "velocityy", "fsl", "maxdepth"]       # the plain targets, as without it
    m = Model(xml, make_sim=_oracle_sim, output_format=".npy", overviews=[("froude", "count", 100)])
    plain = Model(make_newcastle(tmp_path / "plain", duration=120, frequency=60), make_sim=_oracle_sim, output_format=".npy")
    assert not m.device_overviews and plain.overview_list == []
    for model in (m, plain):
        model.scheme.automatic_queue = False                                  # (batch boundaries are not physics-neutral: fixed)
        model.scheme.queue_addition_size = 16
    outs, plain_outs = m.run(), plain.run()
    state = m.sim.download()
    m.close(); plain.close()
    assert len(outs) == len(plain_outs) == 2
    t, last = outs[-1]
    for key, value in [(("depth", "max", 4), "depth"), (("velocityx", "min", 16), "velocityx"), (("froude", "count", 100), "froude")]:
        want = frontend.overview(frontend.derive_output(value, state, m.bed, m.res), key[2], key[1])
        assert np.array_equal(last[key], want) and want.shape == (-(-195 // key[2]), -(-342 // key[2]))
    assert (last[("depth", "max", 4)] > 0).any() and last[("froude", "count", 100)].sum() > 0
    assert np.array_equal(np.load(os.path.join(str(tmp_path / "o"), "output", f"depth4_{int(t)}.npy")), last[("depth", "max", 4)])
    assert np.array_equal(np.load(os.path.join(str(tmp_path / "o"), "output", f"velx16_{int(t)}.npy")), last[("velocityx", "min", 16)])
    # the other targets' files: byte for byte those of the run without overviews
    files = sorted(os.listdir(os.path.join(str(tmp_path / "plain"), "output")))
    assert len(files) == 10
    for f in files:
        assert open(os.path.join(str(tmp_path / "o"), "output", f), "rb").read() == open(os.path.join(str(tmp_path / "plain"), "output", f), "rb").read(), f
    assert len(os.listdir(os.path.join(str(tmp_path / "o"), "output"))) == 14
    for bad, message in (([("depth", "sum", 4)], "unknown aggregate"), ([("bed", "max", 4)], "unknown output"), ([("depth", "max", 0)], "factor")):
        with pytest.raises(ValueError, match=message):
            Model(make_newcastle(tmp_path / "bad", duration=120, frequency=60), make_sim=_oracle_sim, output_format=None, overviews=bad)
