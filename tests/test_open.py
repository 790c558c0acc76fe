"""The open boundary without a GPU: the shared C++ definition of one ring cell's iteration (csrc/hp_open.hpp, in a stand-alone program:
tests/open_probe.cpp) against the NumPy restatement (frontend.Open) bit for bit, the host checks of hp_boundary_add_open, the strips'
selection, the branches and the mass balance of the restatement on the scene both suites use, and the model file's open edges.
The scene (scene()) and the reference run (reference()) are what tests/test_gpu_open.py runs the engine against; the stepwise loop is
tests/test_links.py: StepLoop, unchanged."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import hipims_mi as hp
import oracle
import test_links as T
from conftest import ROOT
from hipims_mi import frontend, strips, synthetic as syn
from test_abi import declared_functions

CSRC = os.path.join(ROOT, "hipims-ocl_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
bits, from_bits = T.bits, T.from_bits

COLS, ROWS, DX = T.COLS, T.ROWS, T.DX
SOUTH, NORTH, WEST, EAST = hp.EDGE_SOUTH, hp.EDGE_NORTH, hp.EDGE_WEST, hp.EDGE_EAST
SEGMENTS = [dict(edge="east", first=6, last=25), dict(edge="south", first=3, last=18)]
REQUIRED = ("inert", "dry", "level_capped", "inward_zeroed", "outflow")     # every branch of frontend.Open.BRANCHES except "inflow"
BATCHES = [1, 7, 20] * 4 + [1, 7]                                           # the 120 iterations both suites run
POOL = 2.6


def scene(real=np.float64, all_wet=False):
    """40 x 32 cells of 2 m: a bed that falls to the east from 2 m to 0.44 m with a channel 0.3 m deep along rows 14-17, a pool at
    2.6 m over columns 1-16, a closed ring -- and the east ring's rows 6..25 and the south ring's columns 3..18 opened again: a real bed,
    2 cm below their inward neighbours'.  Inside the segments: the east ring's row 10 left as a wall; the south ring's column 5 with a
    bed above the pool; a terrace 3 m high over rows 22-25 of the last ten columns, whose cells stay dry, one of them -- the inward
    neighbour of the east ring's row 24 -- disabled; and north-pointing (inward) Qy on row 1 of columns 12-16."""
    y, x = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    bed = 2.0 - 0.04 * x
    bed[14:18, :] -= 0.3
    if not all_wet:
        bed[22:26, 29:39] += 3.0
    bed = syn.round4(bed)
    st = np.zeros((ROWS, COLS, 4))
    st[..., 0] = bed
    st[:, 1:17, 0] = POOL
    if all_wet:
        st[..., 0] = np.maximum(bed + 0.25, st[..., 0])
    st[..., 1] = st[..., 0]
    st[1, 12:17, 3] = 0.3
    syn._walls(st, bed)
    for r in range(6, 26):
        bed[r, COLS - 1] = syn.round4(bed[r, COLS - 2] - 0.02)
    for c in range(3, 19):
        bed[0, c] = syn.round4(bed[1, c] - 0.02)
    st[6:26, COLS - 1, :2] = bed[6:26, COLS - 1, None]
    st[0, 3:19, :2] = bed[0, 3:19, None]
    if not all_wet:
        bed[10, COLS - 1], st[10, COLS - 1] = syn.WALL_BED, 0.0
        bed[0, 5] = st[0, 5, 0] = st[0, 5, 1] = 3.5
        st[24, COLS - 2, 1] = -9999.0
    return st.astype(real), bed.astype(real), np.full((ROWS, COLS), 0.03, real)


def make_open(precision="f64", segments=SEGMENTS, **kw):
    return frontend.Open(ROWS, COLS, DX, oracle.OracleFunctions(precision, dx=DX), segments, **kw)


def interior_volume(st, bed):
    d = np.maximum(0.0, st[1:-1, 1:-1, 0].astype(np.float64) - bed[1:-1, 1:-1].astype(np.float64))
    return math.fsum((d * (DX * DX)).reshape(-1))


@functools.lru_cache(maxsize=None)
def reference(rain=True):
    """The reference run: StepLoop with the rain in front and the open boundary behind, BATCHES iterations; after every batch the state,
    the scalars and the records.  Computed once and shared; nobody changes it."""
    st, bed, man = scene()
    O = make_open()
    loop = T.StepLoop(st, bed, man, ([("uniform", T.RAIN)] if rain else []) + [("open", O)])
    after = []
    for n in BATCHES:
        loop.step(n)
        after.append((loop.download(), loop.scalars(), O.records()))
    for a in after:
        a[0].setflags(write=False)
    return dict(after=after, totals=O.branch_totals(), branches={k: v.copy() for k, v in O.branches.items()}, start=(st, bed, man))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("open") / "open_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "open_probe.cpp")])

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_the_shared_definition_needs_no_hip():
    host = open(os.path.join(CSRC, "hp_open.hpp")).read().split("#ifdef __HIPCC__\n#include")[0]
    code = "\n".join(l.split("//")[0] for l in host.splitlines())
    for name in ("open_impose", "open_record", "validate_open", "open_strip_keeps"):
        assert name in code
    assert "#include <hip" not in code and "__global__" not in code and "hp_math" not in code


def test_abi_additions():
    lib = hp.load_library()
    for name in ("hp_boundary_add_open", "hp_open_read", "hp_open_info"):
        assert name in declared_functions() and hasattr(lib, name) and name in hp.EXPORTS
    assert lib.hp_abi_version() == 2
    assert hp.OPEN_SEGMENT_DTYPE.itemsize == 24 and hp.OPEN_RECORD_DTYPE.itemsize == 32
    seg = hp.pack_open_segments(["east", dict(edge="south", first=3, last=18), (NORTH, 2, 2)], COLS, ROWS)
    assert [tuple(int(v) for v in s) for s in seg] == [(EAST, 0, 1, ROWS - 2), (SOUTH, 0, 3, 18), (NORTH, 0, 2, 2)]


# 2 ---------------------------------------------------------------------------------------------------------------------
def random_cases(n, rng):
    """n random cells, the special ones mixed in: every edge with both signs of Qn, dry and below-bed neighbours, ring beds above the
    neighbour's level, uncounted cells, dt of 0 and negative, zero fluxes, and half of them with values an fp32 domain would hold."""
    c = dict(edge=rng.integers(0, 4, n), bed_i=rng.uniform(-1, 3, n), qn_i=rng.normal(0, 1, n), qs_i=rng.normal(0, 1, n), dt=rng.uniform(1e-4, 2.0, n),
             dx=rng.choice([0.5, 2.0, 3.0, 7.3], n), F=rng.normal(0, 1, n), volume=rng.normal(0, 100, n), active=rng.integers(0, 1000, n).astype(float))
    c["z_i"] = c["bed_i"] + rng.uniform(0, 2, n)
    c["bed_r"] = c["bed_i"] + rng.uniform(-0.5, 0.5, n)
    pick = lambda share: rng.random(n) < share
    m = pick(0.10); c["z_i"][m] = c["bed_i"][m]                                # a dry neighbour
    m = pick(0.04); c["z_i"][m] = c["bed_i"][m] - rng.uniform(0, 1, n)[m]      # ... with a level below its bed
    m = pick(0.10); c["bed_r"][m] = c["z_i"][m] + rng.uniform(0, 1, n)[m]      # the ring's bed above the neighbour's level
    m = pick(0.05); c["bed_r"][m] = c["z_i"][m]
    m = pick(0.08); c["qn_i"][m] = 0.0
    m = pick(0.02); c["qn_i"][m] = -0.0
    m = pick(0.05); c["F"][m] = 0.0
    m = pick(0.04); c["dt"][m] = 0.0
    m = pick(0.04); c["dt"][m] = -0.5
    c["zmax_i"] = np.maximum(c["z_i"], c["z_i"] + rng.uniform(-0.5, 1, n))
    c["zmax_r"] = c["bed_r"] + rng.uniform(-0.5, 2.5, n)
    m = pick(0.03); c["zmax_i"][m] = -9999.0
    m = pick(0.03); c["zmax_r"][m] = -9999.0
    m = pick(0.03); c["bed_r"][m] = 9999.9
    m = pick(0.03); c["bed_i"][m] = 9999.9
    f32 = pick(0.5)
    for f in ("bed_i", "bed_r", "z_i", "zmax_i", "zmax_r", "qn_i", "qs_i", "dt", "dx", "F"):
        c[f][f32] = c[f][f32].astype(np.float32).astype(np.float64)
    return c


def test_the_probe_equals_the_restatement_bit_for_bit(probe):
    n = 6000
    c = random_cases(n, np.random.default_rng(61))
    fields = ("zmax_r", "bed_r", "z_i", "zmax_i", "qn_i", "qs_i", "bed_i", "dt", "dx", "F", "volume", "active")
    got = [l.split() for l in probe([" ".join(["I", str(int(c["edge"][k]))] + [bits(c[f][k]) for f in fields]) for k in range(n)])]
    inert, lvl, qn, qs, dry, capped, zeroed = frontend.Open.impose(c["edge"], c["zmax_r"], c["bed_r"], c["z_i"], c["zmax_i"], c["qn_i"], c["qs_i"], c["bed_i"], c["dt"])
    q_last, volume, active, out = frontend.Open.record(np.full(n, -1.0), c["volume"], c["active"].astype(np.uint64), inert, c["edge"], c["F"], c["dt"], c["dx"])
    q_last = np.where(inert, 0.0, q_last)
    for k in range(n):
        if inert[k]:                                                         # nothing of an inert cell's imposed values is used
            assert got[k][0] == "1" and got[k][8:] == [bits(0.0), bits(c["volume"][k]), str(int(c["active"][k]))], (k, got[k])
            continue
        want = ["0", bits(lvl[k]), bits(np.float32(lvl[k])), bits(qn[k]), bits(qs[k]), str(int(dry[k])), str(int(capped[k])), str(int(zeroed[k])),
                bits(q_last[k]), bits(volume[k]), str(int(active[k]))]
        assert got[k] == want, (k, {f: c[f][k] for f in c}, got[k], want)
    # the cases reached what they were made for: every branch, on every edge, with both signs of Qn
    live = ~inert
    assert inert.sum() > 300 and (inert & (c["dt"] <= 0)).sum() > 100
    for e in (SOUTH, NORTH, WEST, EAST):
        on = live & (c["edge"] == e)
        assert min((on & dry).sum(), (on & capped).sum(), (on & zeroed).sum(), (on & (qn != 0)).sum(), (on & (out > 0)).sum(), (on & (out < 0)).sum()) > 20
        assert (on & ~dry & (c["qn_i"] > 0)).sum() > 100 and (on & ~dry & (c["qn_i"] < 0)).sum() > 100
    assert (live & capped & (c["bed_r"] > c["z_i"])).sum() > 100
    # what the contract promises: the ring never stands above the water that feeds it unless its own bed does, and never takes inward momentum
    assert (lvl[live] <= np.maximum(c["z_i"], c["bed_r"])[live]).all() and (lvl[live] >= c["bed_r"][live]).all()
    positive = (c["edge"] == EAST) | (c["edge"] == NORTH)
    assert (np.where(positive, qn, -qn)[live] >= 0).all() and (qn[live & dry] == 0).all() and (qs[live & dry] == 0).all()


# 3 ---------------------------------------------------------------------------------------------------------------------
def v_line(segments, cols=COLS, rows=ROWS, existing=0, taken=(), count=None):
    words = ["V", cols, rows, existing, len(taken), *taken, len(segments) if count is None else count]
    for s in segments:
        words += [int(s[0]), int(s[1]), int(s[2]), int(s[3])]
    return " ".join(str(w) for w in words)


as_dict = lambda s: dict(edge=s[0], reserved=s[1], first=s[2], last=s[3])
GOOD = (EAST, 0, 6, 25)
BAD = {                                                    # every argument error of the header, and a word of its message
    "unknown edge": ((4, 0, 3, 5), "unknown edge"),
    "negative edge": ((-1, 0, 3, 5), "unknown edge"),
    "reserved": ((SOUTH, 1, 3, 5), "reserved"),
    "first > last": ((SOUTH, 0, 6, 5), "first > last"),
    "corner 0": ((SOUTH, 0, 0, 5), "index 0 "),
    "corner n - 1 (columns)": ((NORTH, 0, 3, COLS - 1), f"index {COLS - 1} "),
    "corner n - 1 (rows)": ((WEST, 0, 3, ROWS - 1), f"index {ROWS - 1} "),
    "negative": ((WEST, 0, -2, 4), "index -2 "),
    "twice": ((EAST, 0, 25, 27), f"cell {25 * COLS + COLS - 1} "),
}


def test_validate_open_rejects_every_argument_error(probe):
    assert probe([v_line([GOOD])]) == ["ok 20"]
    assert probe([v_line([GOOD, (SOUTH, 0, 1, COLS - 2), (NORTH, 0, 1, COLS - 2), (WEST, 0, 1, ROWS - 2)])]) == [f"ok {20 + 2 * (COLS - 2) + ROWS - 2}"]
    for name, (segment, word) in BAD.items():
        out = probe([v_line([GOOD, segment])])[0]
        assert out.startswith("bad ") and "segment 1" in out and word in out, (name, out)
    assert "NULL" in probe([v_line([], count=1)])[0]
    assert "count == 0" in probe([v_line([GOOD], count=0)])[0]
    assert "64 segments" in probe([v_line([(SOUTH, 0, k, k) for k in range(1, 38)] + [(NORTH, 0, k, k) for k in range(1, 29)])])[0]       # 65 at once
    assert "64 segments" in probe([v_line([GOOD], existing=64)])[0]
    assert probe([v_line([GOOD], existing=63)]) == ["ok 20"]
    # a cell an earlier segment of the domain has: the message names the segment and the id
    twice = 7 * COLS + COLS - 1
    out = probe([v_line([(SOUTH, 0, 3, 5), GOOD], existing=1, taken=sorted([2, twice]))])[0]
    assert out.startswith("bad ") and "segment 1" in out and f"cell {twice} " in out, out
    assert probe([v_line([GOOD], existing=1, taken=[1, 2])]) == ["ok 22"]
    # the restatement refuses the same segments
    for name, (segment, _) in BAD.items():
        with pytest.raises(ValueError, match="segment 1"):
            make_open(segments=[as_dict(GOOD), as_dict(segment)])
    with pytest.raises(ValueError, match="64 segments"):
        make_open(segments=[(SOUTH, k, k) for k in range(1, 38)] + [(NORTH, k, k) for k in range(1, 29)])
    with pytest.raises(ValueError):
        make_open(segments=[])
    with pytest.raises(ValueError):
        make_open(segments=None)


@pytest.mark.parametrize("world", [2, 3])
def test_the_strips_selection(probe, world):
    g = strips.ghost_rows(hp.SCHEME_GODUNOV)
    parts = strips.partition(ROWS, world, g)
    whole = [dict(edge=e) for e in ("south", "north", "west", "east")]
    single = make_open(segments=whole)
    owners = np.zeros(len(single.cells), int)
    for own_lo, own_hi, lo, hi in parts:
        O = frontend.Open(hi - lo, COLS, DX, oracle.OracleFunctions("f64", dx=DX), whole, row_offset=lo, global_rows=ROWS)
        got = [int(v) for v in probe([f"S {int(ry)} {int(iy)} {lo} {hi}" for ry, iy in zip(O.ry, O.iy)])]
        assert got == [int(k) for k in O.kept]
        assert np.array_equal(O.cells, single.cells)                          # every strip lists every cell, in the single domain's order
        owners += O.kept & (O.ry >= own_lo) & (O.ry < own_hi)
        # west and east cells on ghost rows are kept; the south and north edges by the strip that stores them
        assert O.kept[(O.edge >= WEST) & (O.ry >= lo) & (O.ry < hi)].all() and not O.kept[(O.edge >= WEST) & ((O.ry < lo) | (O.ry >= hi))].any()
        assert O.kept[O.edge == SOUTH].all() == (lo == 0) and O.kept[O.edge == NORTH].all() == (hi == ROWS)
    assert (owners == 1).all()                                                # every cell's record has exactly one owner


def test_gather_open_takes_every_record_from_the_strip_that_owns_its_row():
    class Engine:
        def add_open(self, segments):
            self.n = getattr(self, "n", 0) + int((segments["last"] - segments["first"] + 1).sum())

        def open_read(self, first=0, count=None):
            rec = np.zeros(self.n, hp.OPEN_RECORD_DTYPE)
            rec["q_last"], rec["volume"], rec["active"] = np.arange(self.n) + 0.5, -np.arange(self.n) - 0.25, np.arange(self.n) + 7
            return rec
    engine = Engine()
    runner = strips.StripRunner(COLS, ROWS, rank=0, world=2, engine_factory=lambda *a: engine, init_process_group=False, loop="torch", exchange_period=1)
    runner.add_open(SEGMENTS)
    runner.add_open(["north"])
    rows = runner.open_rows()
    assert list(rows[:20]) == list(range(6, 26)) and (rows[20:36] == 0).all() and (rows[36:] == ROWS - 1).all()
    sent = []
    theirs = np.flatnonzero(rows >= runner.own_hi)
    runner._gather_parts = lambda mine: (sent.append(mine), [mine, (theirs, engine.open_read()[theirs])])[1]
    got = runner.gather_open()
    assert list(sent[0][0]) == list(np.flatnonzero(rows < runner.own_hi)) and got.tobytes() == engine.open_read().tobytes()
    with pytest.raises(RuntimeError, match="no open segment"):
        strips.StripRunner(COLS, ROWS, rank=0, world=2, engine_factory=lambda *a: Engine(), init_process_group=False, loop="torch", exchange_period=1).gather_open()


# 4, 5 ------------------------------------------------------------------------------------------------------------------
def test_the_scene_is_what_it_says():
    st, bed, _ = scene()
    O = make_open()
    assert len(O.cells) == 36 and list(O.cells[:20]) == [r * COLS + COLS - 1 for r in range(6, 26)] and list(O.cells[20:]) == list(range(3, 19))
    ring = np.ones((ROWS, COLS), bool)
    ring[1:-1, 1:-1] = False
    opened = np.zeros((ROWS, COLS), bool)
    opened.reshape(-1)[O.cells] = True
    assert (bed[ring & ~opened] == syn.WALL_BED).all() and bed[10, COLS - 1] == syn.WALL_BED
    real_bed = opened & (bed < 9999)
    assert real_bed.sum() == 35 and bed[0, 5] > POOL and st[24, COLS - 2, 1] == -9999.0
    assert (st[1, 12:17, 3] > 0).all() and (st[1, 12:17, 0] > bed[1, 12:17]).all()


def test_the_reference_run_takes_every_branch_but_inflow():
    ref = reference()
    assert all(ref["totals"][b] >= 1 for b in REQUIRED), ref["totals"]
    B = ref["branches"]
    assert B["inert"][4] == 120 and B["inert"][18] == 120                      # the wall (east row 10) and the disabled neighbour (east row 24)
    assert B["level_capped"][20 + 2] == 120                                    # the south ring's column 5: its bed above the pool
    assert (B["inward_zeroed"][20 + 9:20 + 14] >= 1).all()                     # the inward Qy on columns 12-16
    assert (B["dry"][[16, 17, 19]] >= 1).all()                                 # the terrace (its row 24 is the inert one)
    state, scalars, rec = ref["after"][-1]
    assert np.isfinite(state).all() and rec["volume"].max() > 1.0 and rec["active"].max() > 100 and rec["active"][4] == 0


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_the_records_balance_the_water_that_left_the_interior():
    """Without rain, over the 120 iterations: what the interior lost and what the records count differ by at most what the flux step may
    snap or zero per cell and step, plus rounding -- and the outflow is a thousand times that, so an edge that lets nothing out fails."""
    ref = reference(rain=False)
    st0, bed, _ = ref["start"]
    state, _, rec = ref["after"][-1]
    lost = interior_volume(st0, bed) - interior_volume(state, bed)
    outflow = math.fsum(rec["volume"])
    iterations, interior, vs = sum(BATCHES), (ROWS - 2) * (COLS - 2), 1e-10
    bound = iterations * interior * 10 * vs * DX * DX + 1e-12 * outflow
    print(f"lost {lost!r} m3, recorded {outflow!r} m3, difference {lost - outflow!r}, bound {bound!r}")
    assert outflow > 1000 * bound
    assert abs(lost - outflow) <= bound


# 7 ---------------------------------------------------------------------------------------------------------------------
MODEL_XML = """<?xml version="1.0"?>
<configuration><metadata><name>open</name></metadata>
<simulation>
  <parameter name="duration" value="2.0"/><parameter name="outputFrequency" value="1.0"/>
  <domainSet><domain type="cartesian" deviceNumber="1">
    <data sourceDir="in" targetDir="out">
      <dataSource type="raster" value="structure,dem" source="dem.asc"/>
      <dataSource type="constant" value="depth" source="1.0"/>
      <dataSource type="constant" value="manningCoefficient" source="0.03"/>
      <dataTarget type="raster" value="depth" format="ASC" target="depth_%t.asc"/>
    </data>
    <scheme name="godunov"><parameter name="courantNumber" value="0.5"/></scheme>
    <boundaryConditions sourceDir="in">
      <domainEdge edge="north" treatment="closed"/><domainEdge edge="west" treatment="closed"/>
      {edges}
    </boundaryConditions>
  </domain></domainSet>
</simulation></configuration>
"""
EDGES = '<domainEdge edge="east" treatment="open" name="outlet" from="3" to="8"/><domainEdge edge="South" treatment="Open"/>'


DEM = syn.round4(1.0 + 0.02 * np.mgrid[0:12, 0:16][0] - 0.02 * np.mgrid[0:12, 0:16][1])      # falls to the east and to the south


def write_model(tmp_path, edges=EDGES):
    os.makedirs(tmp_path / "in", exist_ok=True)
    frontend.write_raster(str(tmp_path / "in" / "dem.asc"), DEM, 2.0)
    xml = tmp_path / "model.xml"
    xml.write_text(MODEL_XML.format(edges=edges))
    return str(xml)


def test_the_model_file_round_trips_its_open_edges(tmp_path):
    cfg = frontend.parse_configuration(write_model(tmp_path))
    assert cfg.closed_edges == {"north", "west"}
    assert cfg.open_edges == [dict(edge="east", name="outlet", first=3, last=8), dict(edge="south", name="south1", first=None, last=None)]
    seg = hp.pack_open_segments(cfg.open_edges, 16, 12)
    assert [tuple(int(v) for v in s) for s in seg] == [(EAST, 0, 3, 8), (SOUTH, 0, 1, 14)]
    _, bed, _, _ = frontend.build_domain(cfg)
    assert (bed[-1, :] == 9999.9).all() and (bed[1:-1, 0] == 9999.9).all()
    assert np.array_equal(bed[1:-1, -1], DEM[1:-1, -1]) and np.array_equal(bed[0, 1:-1], DEM[0, 1:-1])      # an open edge gets no wall
    with pytest.raises(ValueError):
        frontend.parse_configuration(write_model(tmp_path, '<domainEdge edge="up" treatment="open"/>'))


def test_model_hands_its_open_edges_to_the_engine(tmp_path):
    """Model(open_edges=...) and the file's open edges: one call behind the file's boundaries, outflow.csv at every output time with
    math.fsum over each segment's records; an engine without an open boundary is refused."""
    from hipims_mi.model import Model

    class Sim(oracle.OracleSim):
        def add_open(self, segments):
            self.segments = segments.copy()

        def open_read(self):
            rec = np.zeros(int((self.segments["last"] - self.segments["first"] + 1).sum()), hp.OPEN_RECORD_DTYPE)
            rec["volume"], rec["q_last"] = 0.1, 1e-3
            return rec
    make = lambda cls: (lambda cfg, cols, rows, res: cls(cols, rows, dx=res, scheme=cfg.scheme, precision=cfg.precision, end_time=cfg.duration))
    m = Model(write_model(tmp_path), make_sim=make(Sim), open_edges=["north"], output_format=".npy")
    assert [tuple(int(v) for v in s) for s in m.sim.segments] == [(EAST, 0, 3, 8), (SOUTH, 0, 1, 14), (NORTH, 0, 1, 14)]
    m.run()
    rows = open(tmp_path / "out" / "outflow.csv").read().strip().split("\n")
    assert rows[0] == "t,discharge_outlet,volume_outlet,discharge_south1,volume_south1,discharge_north2,volume_north2" and len(rows) == 3
    assert [float(v) for v in rows[-1].split(",")] == [2.0, math.fsum([1e-3] * 6), math.fsum([0.1] * 6), math.fsum([1e-3] * 14), math.fsum([0.1] * 14),
                                                       math.fsum([1e-3] * 14), math.fsum([0.1] * 14)]
    with pytest.raises(NotImplementedError):
        Model(write_model(tmp_path), make_sim=make(oracle.OracleSim))
