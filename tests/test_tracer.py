"""The tracer without a GPU: the shared C++ definition of its fp64 steps (csrc/hp_tracer.hpp, in a stand-alone program:
tests/tracer_probe.cpp) against the NumPy restatement (frontend.Tracer) bit for bit, the host checks of hp_tracer_enable and
hp_tracer_add_source, the restatement's branches and its closed-domain mass on the scene of tests/test_links.py, the model file's
elements and the launch rules (tests/tracer_plan_probe.cpp).  TracedLoop is what tests/test_gpu_tracer.py runs the engine against."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hipims_mi as hp
import oracle
import test_links as T
from conftest import ROOT
from hipims_mi import frontend
from test_abi import declared_functions

CSRC = os.path.join(ROOT, "hipims-ocl_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
bits = lambda v: struct.pack(">d", float(v)).hex()
from_bits = lambda s: struct.unpack(">d", bytes.fromhex(s))[0]
COLS, ROWS, DX = T.COLS, T.ROWS, T.DX
SOURCE = dict(cells=[(8, 8), (9, 8), (25, 20)], series=[(0.0, 0.0), (0.25, 4.0), (5.0, 1.0)])


def blob():
    """M >= 0 in a disc that straddles the scene's wall (columns 19-20): mass on the deep side, on the dry wall and on the shallow side."""
    y, x = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    r2 = (x - 19.5) ** 2 + (y - 14.0) ** 2
    return np.where(r2 < 64.0, 2.0 * np.exp(-r2 / 24.0), 0.0)


def functions(precision, dx=DX):
    return oracle.OracleFunctions(precision, very_small=1e-10, dx=dx)


class TracedLoop(T.StepLoop):
    """T.StepLoop with the tracer behind every boundary and in front of the flux step (the engine's place for it): the tracer is
    the list's last entry, and its apply is handed the loop's own time scalar."""

    def __init__(self, st, bed, man, tracer, boundaries=(), **kw):
        loop = self

        class Behind:
            def apply(self, src, bed_, dt):
                tracer.apply(src, bed_, dt, loop.sc.t)
        super().__init__(st, bed, man, boundaries=tuple(boundaries) + (("tracer", Behind()),), **kw)
        self.tracer = tracer


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tracer") / "tracer_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "tracer_probe.cpp")])

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_the_shared_definition_needs_no_hip():
    host = open(os.path.join(CSRC, "hp_tracer.hpp")).read().split("#ifdef __HIPCC__\n#include")[0]
    code = "\n".join(l.split("//")[0] for l in host.splitlines())
    for name in ("tracer_conc", "tracer_update", "tracer_source_add", "tracer_rate", "validate_tracer_enable", "validate_tracer_source"):
        assert name in code
    assert "#include <hip" not in code and "__global__" not in code and "hp_math" not in code


def test_abi_additions():
    lib = hp.load_library()
    for name in ("hp_tracer_enable", "hp_tracer_disable", "hp_tracer_add_source", "hp_tracer_sources_clear", "hp_tracer_read", "hp_tracer_write",
                 "hp_tracer_info"):
        assert name in declared_functions() and hasattr(lib, name) and name in hp.EXPORTS
    assert lib.hp_abi_version() == 2
    import ctypes as C
    assert C.sizeof(hp.TracerDesc) == 16
    for name in ("tracer_enable", "tracer_disable", "tracer_add_source", "tracer_sources_clear", "tracer_read", "tracer_write", "tracer_info"):
        assert hasattr(hp.Domain, name)
    # argument errors come before any device call: a NULL domain is one, with or without a GPU
    assert lib.hp_tracer_enable(None, None) == -1 and lib.hp_tracer_write(None, None, 0, 0) == -1 and lib.hp_tracer_info(None, None, None, None) == -1
    assert lib.hp_tracer_read(None, None, 0, 0) == -1 and lib.hp_tracer_add_source(None, None, 0, None, 0) == -1


# 2 ---------------------------------------------------------------------------------------------------------------------
def update_cases(n, rng):
    """M, the four neighbours' M, five raw depths (some at or below 1e-10, some negative), four fluxes of both signs (some exactly
    zero), dt and dx."""
    M = rng.uniform(0.0, 5.0, (n, 5)) * (rng.random((n, 5)) > 0.15)
    h = np.where(rng.random((n, 5)) < 0.25, rng.choice([0.0, 1e-10, 9.9e-11, -1e-3, 1.0000001e-10], (n, 5)), 10.0 ** rng.uniform(-9, 1, (n, 5)))
    F = rng.normal(0.0, 1.0, (n, 4)) * 10.0 ** rng.uniform(-6, 1, (n, 4)) * (rng.random((n, 4)) > 0.1)
    dt = 10.0 ** rng.uniform(-4, 0, n)
    dx = rng.choice([1.0, 2.0, 0.3, 7.5, np.float64(np.float32(0.1))], n)
    return M, h, F, dt, dx


def test_the_update_equals_the_restatement_bit_for_bit(probe):
    rng = np.random.default_rng(20261)
    M, h, F, dt, dx = update_cases(4000, rng)
    out = probe(["U " + " ".join(bits(v) for v in (*M[k], *h[k], *F[k], dt[k], dx[k])) for k in range(len(M))])
    c = frontend.Tracer.concentration(M, h)
    seen = set()
    for k in range(len(M)):
        want, masks = frontend.Tracer.update(M[k, 0], c[k, 0], c[k, 1], c[k, 2], c[k, 3], c[k, 4], F[k, 0], F[k, 1], F[k, 2], F[k, 3], dt[k], dx[k])
        assert out[k] == bits(want), (k, from_bits(out[k]), float(want))
        seen |= {name for name, m in masks.items() if bool(m)}
    assert seen == {"e_pos", "e_neg", "w_pos", "w_neg", "n_pos", "n_neg", "s_pos", "s_neg"}
    assert (c == 0.0).any() and (c > 0.0).any()


def test_the_source_step_equals_the_restatement_bit_for_bit(probe):
    rng = np.random.default_rng(20262)
    series = np.array([(0.0, 0.0), (0.25, 4.0), (1.0 / 3.0, -1.0), (5.0, 1.0)])
    lines, want = [], []
    for k in range(600):
        t = float(rng.choice([-1.0, 0.0, 0.25, 5.0, 9.0, rng.uniform(0.0, 5.0)]))
        M, dt, dx = float(rng.uniform(0, 3)), float(10.0 ** rng.uniform(-4, 0)), float(rng.choice([1.0, 2.0, 0.3]))
        n = int(rng.integers(1, len(series) + 1))
        lines.append("S " + " ".join(bits(v) for v in (M, dt, dx, t)) + f" {n} " + " ".join(bits(v) for v in series[:n].reshape(-1)))
        rate = frontend.BedShapes.series_fraction(series[:n], t)
        want.append(bits(rate) + " " + bits(frontend.Tracer.source_step(M, rate, dt, dx)))
    assert probe(lines) == want


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_enable_rejects_every_argument_error(probe):
    ok = "E 0 4 4 " + " ".join(bits(v) for v in (0.0, 1.0, 2.5, 0.0))
    cases = [
        (ok, "ok"),
        ("E 0 4 0", "ok"),
        ("E null", "bad hp_tracer_enable: desc == NULL"),
        ("E 12 4 0", "bad hp_tracer_desc_t size mismatch (ABI)"),
        ("E 0 4 4 " + " ".join(bits(v) for v in (0.0, 1.0, -1e-300, np.nan)), "bad hp_tracer_enable: cell 2: initial must be finite and >= 0"),
        ("E 0 4 4 " + " ".join(bits(v) for v in (0.0, np.inf, 1.0, 1.0)), "bad hp_tracer_enable: cell 1: initial must be finite and >= 0"),
        ("E 0 4 4 " + " ".join(bits(v) for v in (np.nan, 0.0, 1.0, 1.0)), "bad hp_tracer_enable: cell 0: initial must be finite and >= 0"),
    ]
    assert probe([c for c, _ in cases]) == [w for _, w in cases]
    with pytest.raises(ValueError, match="cell 2: initial must be finite and >= 0"):
        frontend.Tracer(2, 2, 1.0, functions("f64"), initial=[[0.0, 1.0], [-1.0, np.nan]])


def test_add_source_rejects_every_argument_error(probe):
    s = lambda *pairs: f"{len(pairs)} " + " ".join(bits(v) for p in pairs for v in p)
    good = s((0.0, 1.0), (10.0, 2.0))
    who = "bad hp_tracer_add_source: "
    cases = [                                                              # an 8 x 6 grid
        (f"A 8 6 0 0 2 9 10 {good}", "ok"),
        (f"A 8 6 0 0 0 {good}", who + "cells / series == NULL"),
        ("A 8 6 0 0 2 9 10 0", who + "cells / series == NULL"),
        (f"A 8 6 0 0 2 9 10 {s((0.0, 1.0), (0.0, 2.0))}", who + "series entry 1: times must be finite and strictly increasing"),
        (f"A 8 6 0 0 2 9 10 {s((np.nan, 1.0))}", who + "series entry 0: times must be finite and strictly increasing"),
        (f"A 8 6 0 0 2 9 10 {s((0.0, 1.0), (1.0, np.inf))}", who + "series entry 1: the mass rate must be finite"),
        (f"A 8 6 0 0 2 9 48 {good}", who + "cell 48 lies outside the grid"),
        (f"A 8 6 0 0 2 9 16 {good}", who + "cell 16 lies on the grid's edge ring"),
        (f"A 8 6 0 0 2 9 15 {good}", who + "cell 15 lies on the grid's edge ring"),
        (f"A 8 6 0 0 2 9 3 {good}", who + "cell 3 lies on the grid's edge ring"),
        (f"A 8 6 0 0 2 9 42 {good}", who + "cell 42 lies on the grid's edge ring"),
        (f"A 8 6 0 0 3 9 10 9 {good}", who + "cell 9 is listed twice"),
        (f"A 8 6 2 10 11 1 2 9 10 {good}", who + "cell 10 is listed twice (another source has it)"),
        (f"A 8 6 1 11 64 2 9 10 {good}", who + "more than 64 sources"),
        (f"A 8 6 1 11 63 2 9 10 {good}", "ok"),
    ]
    assert probe([c for c, _ in cases]) == [w for _, w in cases]
    tr = frontend.Tracer(6, 8, 1.0, functions("f64"))
    tr.add_source([9, 10], [(0.0, 1.0), (10.0, 2.0)])
    for cells, series, what in (([10], [(0.0, 1.0)], "listed twice"), ([16], [(0.0, 1.0)], "edge ring"), ([48], [(0.0, 1.0)], "outside the grid"),
                                ([11], [(0.0, 1.0), (0.0, 1.0)], "strictly increasing"), ([11], [(0.0, np.nan)], "finite")):
        with pytest.raises(ValueError, match=what):
            tr.add_source(cells, series)


# 4 ---------------------------------------------------------------------------------------------------------------------
def traced_scene(enable_all=False, island=True):
    """The scene of tests/test_links.py (its walls, its dry wall, its pedestal, its disabled cell) with the blob; `island`: a dry
    3 x 3 block on the shallow side, whose middle cell and its four neighbours are dry (the scene itself has no such cell: its
    wall is two cells wide); `enable_all`: the disabled cell enabled, so that no face leads into a cell that is never updated."""
    st, bed, man, _ = T.scene()
    if island:
        bed[12:15, 30:33] = st[12:15, 30:33, 0] = st[12:15, 30:33, 1] = 4.0
    if enable_all:
        st[3, 21, 1] = st[3, 21, 0]
    return st, bed, man


def test_the_scene_takes_every_branch():
    """Eight iterations with the cell inflow and a source, towards a target time the fifth iteration reaches: the timestep after
    it is negative (the reference's way of saying that the target is reached), which is the dt <= 0 copy case."""
    st, bed, man = traced_scene()
    tr = frontend.Tracer(ROWS, COLS, DX, functions("f64"), initial=blob())
    tr.add_source(SOURCE["cells"], SOURCE["series"])
    loop = TracedLoop(st, bed, man, tr, boundaries=[("cell", T.INFLOW)], target=0.35)
    loop.step(8)
    totals = tr.branch_totals()
    assert loop.sc.dt < 0 and tr.iterations == 8
    assert all(totals[name] > 0 for name in frontend.Tracer.BRANCHES), totals
    assert tr.branches["disabled"][3, 21] > 0 and tr.branches["dry5"][13, 31] > 0 and tr.branches["ring"][0, 0] == 8
    assert np.isfinite(tr.M).all()


def test_fifty_iterations_keep_the_closed_domain_mass():
    """50 oracle iterations of the scene with closed edges, rain and the cell inflow (water comes in, no tracer does): sum(M) moves
    by no more than the restatement's own rounding.  The bound: what a cell loses through a face its neighbour gains as the same
    product F * c, so the sum changes only by the roundings of a cell's update (the differences, their sum, the quotient by dx, the
    product with dt, the final difference) and of the two sides' face flux: each a relative 2^-53 of a magnitude that the CFL
    condition keeps at or below the largest M, or 2^-52 * max(M) a cell and iteration with room for all of them to be counted at
    half weight: cells * iterations * 2^-52 * max(M), max(M) the largest M met in the run.  Derived, not tuned."""
    st, bed, man = traced_scene(enable_all=True)
    m0 = blob()
    tr = frontend.Tracer(ROWS, COLS, DX, functions("f64"), initial=m0)
    loop = TracedLoop(st, bed, man, tr, boundaries=[("uniform", T.RAIN), ("cell", T.INFLOW)])
    largest = float(m0.max())
    for _ in range(50):
        loop.step(1)
        largest = max(largest, float(np.abs(tr.M).max()))
    import math
    before, after = math.fsum(m0.reshape(-1)), math.fsum(tr.M.reshape(-1))
    bound = ROWS * COLS * 50 * 2.0 ** -52 * largest
    print(f"sum(M): {before!r} -> {after!r}, change {after - before:.3e}, bound {bound:.3e}, largest M {largest!r}")
    assert tr.branch_totals()["moved"] > 40 * 1000 and not np.array_equal(tr.M, m0)
    assert abs(after - before) <= bound


def test_the_loop_with_an_empty_tracer_is_the_oracle_in_every_bit():
    """The tracer reads the state and writes only M: the traced loop's water is the untraced loop's."""
    st, bed, man = traced_scene()
    tr = frontend.Tracer(ROWS, COLS, DX, functions("f64"), initial=blob())
    a = TracedLoop(st, bed, man, tr, boundaries=[("uniform", T.RAIN)])
    b = T.StepLoop(st, bed, man, boundaries=[("uniform", T.RAIN)])
    a.step(3)
    b.step(3)
    assert np.array_equal(a.download(), b.download()) and a.scalars() == b.scalars()


def test_concentration_output():
    st, bed, _ = traced_scene()
    M = blob()
    c = frontend.tracer_concentration(M, st, bed)
    h = st[..., 0] - bed
    assert (c[h <= 1e-8] == -9999.0).all() and (h <= 1e-8).any()
    assert np.array_equal(c[h > 1e-8], M[h > 1e-8] / h[h > 1e-8])


# 5 ---------------------------------------------------------------------------------------------------------------------
MODEL_XML = """<?xml version="1.0"?>
<configuration><metadata><name>tracer</name></metadata>
<simulation>
  <parameter name="duration" value="2.0"/><parameter name="outputFrequency" value="1.0"/>
  <domainSet><domain type="cartesian" deviceNumber="1">
    <data sourceDir="in" targetDir="out">
      <dataSource type="raster" value="structure,dem" source="dem.asc"/>
      <dataSource type="constant" value="depth" source="1.0"/>
      <dataSource type="constant" value="manningCoefficient" source="0.03"/>
      <dataSource type="raster" value="tracer" source="m0.asc"/>
      <tracerSource mapFile="cells.csv" source="rate.csv"/>
      <dataTarget type="raster" value="depth" format="ASC" target="depth_%t.asc"/>
      <dataTarget type="raster" value="tracer" format="ASC" target="tracer_%t.asc"/>
      <dataTarget type="raster" value="concentration" format="ASC" target="conc_%t.asc"/>
    </data>
    <scheme name="{scheme}"><parameter name="courantNumber" value="0.5"/></scheme>
    <boundaryConditions sourceDir="in">
      <domainEdge edge="north" treatment="closed"/><domainEdge edge="south" treatment="closed"/>
      <domainEdge edge="east" treatment="closed"/><domainEdge edge="west" treatment="closed"/>
    </boundaryConditions>
  </domain></domainSet>
</simulation></configuration>
"""
FILE_SOURCE = dict(cells=[(3, 3), (4, 3)], series=[(0.0, 1.0 / 3.0), (2.0, 1.0)])


def write_model(tmp_path, scheme="godunov"):
    os.makedirs(tmp_path / "in", exist_ok=True)
    frontend.write_raster(str(tmp_path / "in" / "dem.asc"), np.zeros((12, 16)), 2.0)
    m0 = np.zeros((12, 16))
    m0[5:8, 6:10] = 1.5
    frontend.write_raster(str(tmp_path / "in" / "m0.asc"), m0, 2.0)
    frontend.write_tracer_source_csv(str(tmp_path / "in" / "cells.csv"), str(tmp_path / "in" / "rate.csv"), FILE_SOURCE["cells"], FILE_SOURCE["series"])
    xml = tmp_path / "model.xml"
    xml.write_text(MODEL_XML.format(scheme=scheme))
    return str(xml), m0


def test_the_model_file_elements_parse(tmp_path):
    xml, _ = write_model(tmp_path)
    cfg = frontend.parse_configuration(xml)
    assert any("tracer" in src[1] and src[0] == "raster" and src[2] == "m0.asc" for src in cfg.sources)
    assert len(cfg.tracer_sources) == 1
    assert cfg.tracer_sources[0]["cells"] == FILE_SOURCE["cells"]
    assert np.array_equal(cfg.tracer_sources[0]["series"], np.array(FILE_SOURCE["series"]))        # (repr round-trips 1 / 3)
    assert [what for what, _ in cfg.targets] == ["depth", "tracer", "concentration"]


def test_model_hands_its_tracer_to_the_engine(tmp_path):
    """The file's raster and <tracerSource>, or Model(tracer=...): enabled behind the boundaries, M and M / h written at every
    output time; an engine without a tracer is refused, and so is a tracer target without a tracer."""
    from hipims_mi.model import Model

    class Sim(oracle.OracleSim):
        def tracer_enable(self, initial=None):
            self.m = np.zeros((self.rows, self.cols)) if initial is None else np.array(initial)
            self.tracer_sources = []

        def tracer_add_source(self, cells, series):
            self.tracer_sources.append((list(cells), np.array(series)))

        def tracer_read(self):
            return self.m.copy()
    make = lambda cls: (lambda cfg, cols, rows, res: cls(cols, rows, dx=res, scheme=cfg.scheme, precision=cfg.precision, end_time=cfg.duration))
    xml, m0 = write_model(tmp_path)
    m = Model(xml, make_sim=make(Sim), output_format=".npy")
    assert np.array_equal(m.sim.m, m0) and len(m.sim.tracer_sources) == 1 and m.sim.tracer_sources[0][0] == FILE_SOURCE["cells"]
    m.run()
    got = np.load(tmp_path / "out" / "tracer_2.npy")
    assert np.array_equal(got, m0)
    conc = np.load(tmp_path / "out" / "conc_2.npy")
    assert np.array_equal(conc, frontend.tracer_concentration(m0, m.sim.download(), m.bed))
    more = dict(initial=None, sources=[dict(cells=[(5, 5)], series=[(0.0, 2.0)])])
    m = Model(xml, make_sim=make(Sim), tracer=more, output_format=".npy")
    assert not m.sim.m.any() and m.sim.tracer_sources[0][0] == [(5, 5)]
    with pytest.raises(NotImplementedError):
        Model(xml, make_sim=make(oracle.OracleSim))
    bare = tmp_path / "bare.xml"
    bare.write_text(MODEL_XML.format(scheme="godunov").replace('<dataSource type="raster" value="tracer" source="m0.asc"/>', "")
                    .replace('<tracerSource mapFile="cells.csv" source="rate.csv"/>', ""))
    with pytest.raises(ValueError, match="needs a tracer"):
        Model(str(bare), make_sim=make(Sim))


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_a_traced_domain_never_pairs_and_never_speculates(tmp_path):
    exe = tmp_path / "tracer_plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function", "-O1", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "tracer_plan_probe.cpp")])
    words = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(words[0::2], (int(w) for w in words[1::2])))
    assert got["checked"] > 1000 and got["traced_pairs"] == 0 and got["traced_spec"] == 0
    assert got["plain_pairs"] > 0 and got["plain_spec"] > 0
