"""The probe recorder without a GPU: frontend.rasterise_section's paths and weights, the NumPy restatement
(frontend.ProbeRecorder, the reference the GPU tests hold the device kernel to) on hand-made states and against a plain Python
loop of the kernel's summation order, the six hp_probes_* entry points and their descriptor, the model file's <gauge> and
<section> elements, and a world-2 strip run over gloo with the oracle engine.  No tolerances anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hipims_mi as hp
import oracle
from hipims_mi import frontend, strips, synthetic as syn
from model_dir import make_newcastle
from test_abi import HEADER, declared_functions

ND = frontend.NODATA
PROBE_FUNCTIONS = ["hp_probes_disable", "hp_probes_enable", "hp_probes_info", "hp_probes_read", "hp_probes_reset", "hp_probes_sample"]
SEGMENTS = [((3, 4), (17, 4)), ((5, 2), (5, 19)), ((0, 0), (9, 9)), ((2, 3), (30, 8)), ((4, 1), (7, 25)), ((30, 8), (2, 3)),
            ((7, 25), (4, 1)), ((9, 0), (0, 9)), ((17, 4), (3, 4)), ((1, 1), (2, 1)), ((6, 6), (6, 5)), ((0, 10), (13, 3))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def loop_discharge(terms, dx):
    """record_probes' order in plain Python floats: strided partial sums from +0.0, the halving tree, one multiply."""
    part = [0.0] * 256
    for j in range(256):
        for k in range(j, len(terms), 256):
            part[j] = part[j] + float(terms[k])
    s = 128
    while s > 0:
        for i in range(s):
            part[i] = part[i] + part[i + s]
        s >>= 1
    return dx * part[0]


# ---- rasterise_section ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p0,p1", SEGMENTS)
def test_rasterise_section_path_and_weights(p0, p1):
    sec = frontend.rasterise_section(p0, p1)
    again = frontend.rasterise_section(p0, p1)
    assert all(np.array_equal(a, b) for a, b in zip(sec, again))                   # deterministic
    cells, wx, wy = sec
    (x0, y0), (x1, y1) = p0, p1
    assert cells.shape == (abs(x1 - x0) + abs(y1 - y0) + 1, 2) and wx.dtype == wy.dtype == np.int8
    assert tuple(cells[0]) == p0 and tuple(cells[-1]) == p1
    steps = np.diff(cells, axis=0)
    assert (np.abs(steps).sum(axis=1) == 1).all()                                  # 4-connected
    assert (steps[:, 0] * np.sign(x1 - x0) >= 0).all() and (steps[:, 1] * np.sign(y1 - y0) >= 0).all()    # monotone
    # every cell centre within one cell width of the straight segment
    d = np.array([x1 - x0, y1 - y0], float)
    rel = cells - np.array(p0)
    along = np.clip(rel @ d / (d @ d), 0.0, 1.0)
    assert np.hypot(*(rel - along[:, None] * d).T).max() < 1.0
    # a step (tx, ty) belongs to the cell it leaves and carries the left normal (-ty, tx); the last cell carries nothing
    assert np.array_equal(wx[:-1], -steps[:, 1]) and np.array_equal(wy[:-1], steps[:, 0]) and wx[-1] == wy[-1] == 0
    assert len(wx) == len(wy) == len(cells)


def test_rasterise_section_tie_goes_to_x():
    assert [tuple(c) for c in frontend.rasterise_section((0, 0), (2, 2)).cells] == [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2)]


# ---- ProbeRecorder ---------------------------------------------------------------------------------------------------------
def uniform_field(cols, rows, a, b, depth=1.0):
    st = np.zeros((rows, cols, 4))
    st[..., 0] = st[..., 1] = depth
    st[..., 2], st[..., 3] = a, b
    return st, np.zeros((rows, cols))


@pytest.mark.parametrize("p0,p1", SEGMENTS)
def test_uniform_field_discharge_is_exact(p0, p1):
    a, b, dx = 3.0, -5.0, 2.0
    st, bed = uniform_field(32, 32, a, b)
    rec = frontend.ProbeRecorder([], [frontend.rasterise_section(p0, p1)], dx=dx)
    rec.record(st, bed, 1.5)
    out = rec.series()
    assert out["t"].tolist() == [1.5] and out["gauges"].shape == (1, 0, 4) and out["sections"].shape == (1, 1)
    assert out["sections"][0, 0] == dx * (b * (p1[0] - p0[0]) - a * (p1[1] - p0[1]))


def test_closed_rectangle_sums_to_zero():
    st, bed = uniform_field(40, 30, 3.0, -5.0)              # small integers, dx = 2: every term and every sum is exact
    corners = [(4, 3), (33, 3), (33, 25), (4, 25)]
    secs = [frontend.rasterise_section(corners[k], corners[(k + 1) % 4]) for k in range(4)]
    rec = frontend.ProbeRecorder([], secs, dx=2.0)
    rec.record(st, bed, 0.0)
    q = rec.series()["sections"][0]
    assert q.tolist() == [-290.0, -132.0, 290.0, 132.0] and q.sum() == 0.0


def test_dry_and_uncounted_cells():
    cols, rows = 8, 6
    st, bed = uniform_field(cols, rows, 2.0, 1.0, depth=1.0)
    st[1, 1] = (5.0, -9999.0, 2.0, 1.0)                       # disabled
    bed[1, 2] = 9999.9; st[1, 2, :2] = 10001.0                # a wall with water on it
    st[1, 3, :2] = 0.0                                        # dry (Z == bed), discharge left in place
    st[1, 4, :2] = 1e-8                                       # exactly at the wet threshold: not wet
    bed[1, 5] = 2.0                                           # Z < bed: negative depth
    gauges = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (6, 1)]
    dead = frontend.Section(np.array([(x, 1) for x in range(1, 6)]), np.ones(5, np.int8), np.ones(5, np.int8))
    mixed = frontend.Section(np.array([(x, 1) for x in range(0, 8)]), -np.ones(8, np.int8), np.zeros(8, np.int8))
    rec = frontend.ProbeRecorder(gauges, [dead, mixed], dx=2.0)
    rec.record(st, bed, 7.0)
    rec.record(st.astype(np.float32), bed.astype(np.float32), 8.0)       # fp32 inputs are widened first
    out = rec.series()
    g = out["gauges"][0]
    assert (g[0] == ND).all() and (g[1] == ND).all()                     # not counted: NODATA in all four
    assert g[2].tolist() == [0.0, 0.0, 2.0, 1.0]                         # dry but counted: raw values, no wet test
    assert g[3].tolist() == [1e-8, 1e-8, 2.0, 1.0]
    assert g[4].tolist() == [1.0, -1.0, 2.0, 1.0]                        # depth is not clamped
    assert g[5].tolist() == [1.0, 1.0, 2.0, 1.0] and np.array_equal(g[5], g[6])       # the same cell twice
    assert bits(out["sections"][0, 0]) == bits(0.0)                      # +0.0, not -0.0, although wx * Qx would be negative ...
    assert out["sections"][0, 1] == 2.0 * (-2.0 * 3)                     # ... and the three live cells of the second
    assert np.array_equal(out["gauges"][1][5], g[5]) and out["sections"][1, 1] == out["sections"][0, 1]
    assert out["t"].tolist() == [7.0, 8.0]
    neg = frontend.Section(np.array([(1, 1), (2, 1)]), -np.ones(2, np.int8), np.zeros(2, np.int8))
    rec = frontend.ProbeRecorder([], [neg], dx=-1.0)
    rec.record(st, bed, 0.0)
    assert bits(rec.series()["sections"][0, 0]) == bits(-0.0)            # dx * (+0.0) with dx < 0: the one multiply, as it rounds
    for bad in ([(np.array([(1, 1)]), [1], [0])], [(np.array([(1, 1), (2, 1)]), [2, 0], [0, 0])], [(np.array([(1, 1), (2, 1)]), [1], [0, 0])]):
        with pytest.raises(ValueError):
            frontend.ProbeRecorder([], bad)


@pytest.mark.parametrize("m", [2, 255, 256, 257, 513])
def test_summation_order_against_a_plain_loop(m):
    rng = np.random.default_rng(m)
    cols, rows = 23, 19
    st = np.zeros((rows, cols, 4))
    st[..., 0] = st[..., 1] = rng.uniform(0.5, 2.0, (rows, cols))
    st[..., 2:] = rng.normal(0.0, 1.0, (rows, cols, 2)) * 10.0 ** rng.integers(-6, 7, (rows, cols, 1))
    bed = np.zeros((rows, cols))
    dry = rng.random((rows, cols)) < 0.2
    st[dry, 0] = 0.0
    cells = np.stack([rng.integers(0, cols, m), rng.integers(0, rows, m)], axis=1)       # (cells are revisited)
    wx, wy = rng.integers(-1, 2, m).astype(np.int8), rng.integers(-1, 2, m).astype(np.int8)
    dx = 1.7
    rec = frontend.ProbeRecorder([], [(cells, wx, wy)], dx=dx)
    rec.record(st, bed, 0.0)
    terms = []
    for (x, y), a, b in zip(cells, wx, wy):
        z, _, qx, qy = (float(v) for v in st[y, x])
        terms.append(float(a) * qx + float(b) * qy if z - 0.0 > 1e-8 else 0.0)
    want = loop_discharge(terms, dx)
    assert bits(rec.series()["sections"][0, 0]) == bits(want)
    assert bits(frontend.fold_section_terms(terms, dx)) == bits(want)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_six_entry_points():
    lib = hp.load_library()
    assert [n for n in declared_functions() if n.startswith("hp_probes_")] == PROBE_FUNCTIONS
    for n in PROBE_FUNCTIONS:
        assert hasattr(lib, n) and n in hp.EXPORTS
    text = open(HEADER).read()
    assert "#define HP_ABI_VERSION 2" in text and lib.hp_abi_version() == 2
    assert "no reference counterpart: HiPIMS-OCL writes rasters only" in text
    # the descriptor: the header's fields in the header's order, at the offsets of the C layout (natural alignment)
    body = re.search(r"typedef struct \{([^}]*)\} hp_probes_desc_t;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t.replace(" ", ""), n) for t, n in re.findall(r"((?:const\s+)?\w+\s*\*?)\s*(\w+);", body)]
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "constuint64_t*": C.POINTER(C.c_uint64), "constint8_t*": C.POINTER(C.c_int8)}
    assert [n for _, n in fields] == [n for n, _ in hp.ProbesDesc._fields_]
    offset = 0
    for (t, n), (_, py) in zip(fields, hp.ProbesDesc._fields_):
        assert py is ctype[t] or py == ctype[t], (n, t, py)
        size = C.sizeof(ctype[t])
        offset = -(-offset // size) * size
        assert getattr(hp.ProbesDesc, n).offset == offset and getattr(hp.ProbesDesc, n).size == size, n
        offset += size
    assert C.sizeof(hp.ProbesDesc) == -(-offset // 8) * 8 == 64


def test_argument_errors_come_before_any_device_use():
    lib = hp.load_library()

    def invalid(rc, message):
        assert rc == -1, (rc, message, lib.hp_last_error())
        assert message.encode() in lib.hp_last_error(), (message, lib.hp_last_error())

    g = np.array([0, 1], np.uint64)
    off = np.array([0, 2], np.uint64)
    cells = np.array([3, 4], np.uint64)
    w = np.array([1, 0], np.int8)
    P64, P8 = C.POINTER(C.c_uint64), C.POINTER(C.c_int8)

    def desc(size=C.sizeof(hp.ProbesDesc), capacity=4, gauges=2, sections=1, offsets=off, gauge_cells=g):
        d = hp.ProbesDesc(size, capacity, gauges, gauge_cells.ctypes.data_as(P64) if gauge_cells is not None else None, sections,
                          offsets.ctypes.data_as(P64), cells.ctypes.data_as(P64), w.ctypes.data_as(P8), w.ctypes.data_as(P8))
        return C.byref(d)

    invalid(lib.hp_probes_enable(None, None), "desc == NULL")
    invalid(lib.hp_probes_enable(None, desc(size=56)), "size mismatch")
    invalid(lib.hp_probes_enable(None, desc(capacity=0)), "capacity")
    invalid(lib.hp_probes_enable(None, desc(gauges=65537)), "65536 gauges")
    invalid(lib.hp_probes_enable(None, desc(sections=1025)), "1024 sections")
    invalid(lib.hp_probes_enable(None, desc(gauges=0, sections=0)), "neither a gauge nor a section")
    invalid(lib.hp_probes_enable(None, desc(gauge_cells=None)), "gauge_cells == NULL")
    invalid(lib.hp_probes_enable(None, desc(capacity=2 ** 22 + 1, gauges=0, sections=7)), "256 MiB")      # stride 8: 64 B a record
    invalid(lib.hp_probes_enable(None, desc()), "null domain")
    for f in (lib.hp_probes_disable, lib.hp_probes_reset, lib.hp_probes_sample):
        invalid(f(None), "null domain")
    n = C.c_uint64(0)
    invalid(lib.hp_probes_info(None, C.byref(n), C.byref(n), C.byref(n)), "null domain")
    buf = np.zeros(8)
    invalid(lib.hp_probes_read(None, 0, 1, buf.ctypes.data_as(C.POINTER(C.c_double))), "null domain")


# ---- the front end ---------------------------------------------------------------------------------------------------------
def _with_probes(xml):
    text = open(xml).read()
    marker = '<dataTarget type="raster" value="maxdepth" format="HFA" target="maxdepth_%t.img" />'
    assert marker in text
    open(xml, "w").write(text.replace(marker, marker + '\n<gauge name="quay" x="120" y="60"/>\n<gauge name="hill" x="300" y="150" />'
                                      '\n<section name="street" x0="100" y0="80" x1="180" y1="110"/>'))
    return xml


def test_model_file_elements(tmp_path):
    plain = frontend.parse_configuration(make_newcastle(tmp_path / "plain"))
    probed = frontend.parse_configuration(_with_probes(make_newcastle(tmp_path / "probed")))
    assert plain.gauges == [] and plain.sections == []
    assert probed.gauges == [("quay", 120, 60), ("hill", 300, 150)] and probed.sections == [("street", 100, 80, 180, 110)]
    # everything else is what it was: the elements change nothing a model file without them has
    a, b = vars(plain).copy(), vars(probed).copy()
    for cfg in (a, b):
        for key in ("gauges", "sections", "source_dir", "target_dir"):
            cfg.pop(key)
        cfg["boundaries"] = [(x.kind, x.name, x.value, x.series.tolist()) for x in cfg["boundaries"]]
    assert a == b


def _oracle_sim(cfg, cols, rows, res):
    return oracle.OracleSim(cols, rows, dx=res, scheme=cfg.scheme, very_small=cfg.dry_threshold, courant=cfg.courant,
                            end_time=cfg.duration, friction=cfg.friction, threads=4)


def test_model_records_on_the_oracle_engine(tmp_path):
    from hipims_mi.model import Model
    runs = {}
    for tag in ("plain", "probed"):
        xml = make_newcastle(tmp_path / tag, duration=600, frequency=30)
        m = Model(_with_probes(xml) if tag == "probed" else xml, make_sim=_oracle_sim, output_format=".npy",
                  sections={"kw": ((10, 10), (10, 40))} if tag == "probed" else None)
        m.scheme.automatic_queue = False                   # (batch boundaries are not physics-neutral: fixed)
        m.scheme.queue_addition_size = 25
        if tag == "plain":
            assert m.scheme.samplers == [] and m.probes() is None and m.host_probes is None
        else:
            assert m.host_probes is not None and not m.device_probes and len(m.scheme.samplers) == 1
        outs = m.run(max_outputs=2)
        runs[tag] = (outs, m.sim.download(), m.sim.scalars(), m.probes(), m.scheme.iterations, m.bed)
        m.close()
    plain, probed = runs["plain"], runs["probed"]
    assert np.array_equal(plain[1], probed[1]) and plain[2] == probed[2]                 # the run is the run without probes
    for (_, a), (_, b) in zip(plain[0], probed[0]):
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    series = probed[3]
    n = probed[4] // 25
    assert series["t"].shape == (n,) and series["gauges"].shape == (n, 2, 4) and series["sections"].shape == (n, 2)
    assert (np.diff(series["t"]) >= 0).all() and series["t"][-1] == probed[2]["t"]
    final, bed = probed[1], probed[5]
    assert series["gauges"][-1, 0].tolist() == [final[60, 120, 0], final[60, 120, 0] - bed[60, 120], final[60, 120, 2], final[60, 120, 3]]
    assert (series["sections"] != 0).any()
    out = os.path.join(str(tmp_path / "probed"), "output")
    assert not os.path.exists(os.path.join(str(tmp_path / "plain"), "output", "gauges.csv"))
    lines = open(os.path.join(out, "gauges.csv")).read().splitlines()
    assert lines[0] == "time,name,fsl,depth,qx,qy" and len(lines) == 1 + 2 * n
    assert lines[-1] == ",".join([repr(float(series["t"][-1])), "hill"] + [repr(float(v)) for v in series["gauges"][-1, 1]])
    lines = open(os.path.join(out, "sections.csv")).read().splitlines()
    assert lines[0] == "time,name,discharge" and len(lines) == 1 + 2 * n
    assert lines[1] == f"{float(series['t'][0])!r},street,{float(series['sections'][0, 0])!r}" and lines[2].split(",")[1] == "kw"
    with pytest.raises(ValueError, match="outside the domain"):
        Model(make_newcastle(tmp_path / "bad"), make_sim=_oracle_sim, gauges=[("g", 342, 0)])


# ---- strips over gloo ------------------------------------------------------------------------------------------------------
STRIP_CASE = dict(cols=40, rows=36, batches=(7, 9, 4, 10), gauges=[(5, 16), (30, 17), (7, 18), (33, 19), (12, 2)],
                  sections=[((3, 4), (36, 31)), ((20, 30), (20, 5))])


def _strip_worker(rank, world, port, q):
    import functools
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from strip_oracle_engine import OracleStripEngine
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    c = STRIP_CASE
    st, bed, man = syn.s_rough(c["cols"], c["rows"], manning=None)
    r = strips.StripRunner(c["cols"], c["rows"], rank=rank, world=world,
                           engine_factory=functools.partial(OracleStripEngine, scheme=strips.SCHEME_GODUNOV))
    r.upload_global(st, bed, man)
    r.set_target_time(1e9)
    r.probes_enable(c["gauges"], [frontend.rasterise_section(*s) for s in c["sections"]], dx=1.0)
    for n in c["batches"]:
        r.step(n)
        r.probes_sample()
    got = r.gather_probes()
    if rank == 0:
        q.put(got)
    else:
        assert got is None
    r.close()


def test_strip_runner_gathers_probes_over_gloo():
    import torch.multiprocessing as mp
    from test_strips_gloo import _free_port
    c = STRIP_CASE
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_strip_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    st, bed, man = syn.s_rough(c["cols"], c["rows"], manning=None)
    single = oracle.OracleSim(c["cols"], c["rows"], quirks=oracle.QUIRKS_REFERENCE & ~oracle.Q6_MUSCL_SERIAL)
    single.upload(st, bed, man)
    single.set_target(1e9)
    secs = [frontend.rasterise_section(*s) for s in c["sections"]]
    cut = strips.partition(c["rows"], 2, 1)[0][1]
    assert all(s.cells[:, 1].min() < cut <= s.cells[:, 1].max() for s in secs)           # every section crosses the cut
    assert {y >= cut for _, y in c["gauges"]} == {False, True}                          # a gauge in each strip
    ref = frontend.ProbeRecorder(c["gauges"], secs, dx=1.0)
    for n in c["batches"]:
        single.run(n)
        ref.record(single.download(), bed, single.scalars()["t"])
    want = ref.series()
    assert want["t"][-1] > 0 and (want["sections"] != 0).any() and (want["gauges"] != ND).any()
    for key in ("t", "gauges", "sections"):
        assert got[key].shape == want[key].shape and np.array_equal(bits(got[key]), bits(want[key])), key
