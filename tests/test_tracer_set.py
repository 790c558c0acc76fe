"""The tracer set without a GPU: the shared C++ definition of step 6 and of the per-species source step (csrc/hp_tracer.hpp, in a
stand-alone program: tests/tracer_set_probe.cpp) against the NumPy restatement (frontend.Tracer(decay=...)) bit for bit, the host
checks of hp_tracer_enable_set and hp_tracer_add_source_to, frontend.TracerSet against K separate Tracers on the scene of
tests/test_links.py, and the model file's elements."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hipims_mi as hp
import oracle
import test_links as T
import test_tracer as TT
from hipims_mi import frontend
from test_abi import declared_functions
from test_tracer import CSRC, HERE, bits, from_bits

COLS, ROWS, DX = T.COLS, T.ROWS, T.DX
SOURCE_2 = dict(cells=[(9, 8), (30, 12)], series=[(0.0, 2.0), (1.0, 0.5)])   # shares (9, 8) with TT.SOURCE: another species may


def planes():
    """Three initial rasters: the blob, zeros, and a gradient on the shallow side."""
    y, x = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    return np.stack([TT.blob(), np.zeros((ROWS, COLS)), np.where(x > 21, 0.125 + x / 64.0 + y / 128.0, 0.0)])


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tracer_set") / "tracer_set_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "tracer_set_probe.cpp")])

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_the_shared_definition_needs_no_hip():
    host = open(os.path.join(CSRC, "hp_tracer.hpp")).read().split("#ifdef __HIPCC__\n#include")[0]
    code = "\n".join(l.split("//")[0] for l in host.splitlines())
    for name in ("tracer_decay", "validate_tracer_set_enable", "validate_tracer_source"):
        assert name in code
    assert "#include <hip" not in code and "__global__" not in code and "hp_math" not in code
    kernels = open(os.path.join(CSRC, "hp_tracer.hpp")).read().split("#ifdef __HIPCC__\n#include")[1]
    assert "tracer_step_set" in kernels and kernels.count("tracer_decay(") >= 2       # the kernel's two exits use the shared step 6


def test_abi_additions():
    lib = hp.load_library()
    for name in ("hp_tracer_enable_set", "hp_tracer_add_source_to", "hp_tracer_read_species", "hp_tracer_write_species", "hp_tracer_set_info"):
        assert name in declared_functions() and hasattr(lib, name) and name in hp.EXPORTS
    assert lib.hp_abi_version() == 2
    assert C.sizeof(hp.TracerSetDesc) == 24 and hp.TRACER_MAX_SPECIES == 8 == frontend.Tracer.MAX_SPECIES
    for name in ("tracer_enable_set", "tracer_set_info"):
        assert hasattr(hp.Domain, name)
    # argument errors come before any device call: a NULL domain is one, with or without a GPU
    assert lib.hp_tracer_enable_set(None, None) == -1 and lib.hp_tracer_set_info(None, None, None) == -1
    assert lib.hp_tracer_read_species(None, 0, None, 0, 0) == -1 and lib.hp_tracer_write_species(None, 0, None, 0, 0) == -1
    assert lib.hp_tracer_add_source_to(None, 0, None, 0, None, 0) == -1


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_the_decay_equals_the_restatement_bit_for_bit(probe):
    """Random cases, and the grid lambda * dt in {0, tiny, 1, huge} x M in {0, denormal, large}."""
    rng = np.random.default_rng(20281)
    cases = [(float(m), float(l), float(dt)) for m, l, dt in zip(rng.uniform(0, 5, 3000) * (rng.random(3000) > 0.1), 10.0 ** rng.uniform(-8, 4, 3000),
                                                                  10.0 ** rng.uniform(-5, 1, 3000))]
    for M in (0.0, 5e-324, 2.5e-310, 1e300, 1.7976931348623157e308):
        for lam, dt in ((0.0, 0.5), (1e-300, 1e-20), (2.0 ** -60, 1.0), (4.0, 0.25), (1.0, 1.0), (1e200, 1e100), (1e308, 1e308), (3.0, 0.0), (3.0, -1.0)):
            cases.append((M, lam, dt))
    out = probe(["D " + " ".join(bits(v) for v in c) for c in cases])
    divided = 0
    for (M, lam, dt), got in zip(cases, out):
        want = frontend.Tracer.decay_step(M, lam, dt)
        assert got == bits(want), (M, lam, dt, from_bits(got), float(want))
        if not (lam > 0 and dt > 0):
            assert got == bits(M)                                          # nothing is divided: the bits of the single tracer
        else:
            divided += 1
            assert 0.0 <= from_bits(got) <= M                              # implicit Euler never overshoots zero
    assert divided > 3000
    assert frontend.Tracer.decay_step(1.0, 1.0, 1.0) == 0.5 and frontend.Tracer.decay_step(1e300, 1e308, 1e308) == 0.0


def test_the_source_step_of_a_species_equals_the_restatement_bit_for_bit(probe):
    """A listed cell on a copy case (still water): the source step, then step 6, as one species' plane sees the iteration."""
    rng = np.random.default_rng(20282)
    series = np.array([(0.0, 0.0), (0.25, 4.0), (1.0 / 3.0, -1.0), (5.0, 1.0)])
    fn = TT.functions("f64", dx=2.0)
    lines, want = [], []
    for k in range(300):
        t = float(rng.choice([-1.0, 0.0, 0.25, 5.0, 9.0, rng.uniform(0.0, 5.0)]))
        M, dt, lam = float(rng.uniform(0, 3)), float(rng.choice([10.0 ** rng.uniform(-4, 0), 0.0, -1.0])), float(rng.choice([0.0, 1e-6, 0.5, 1e3]))
        n = int(rng.integers(1, len(series) + 1))
        lines.append("S " + " ".join(bits(v) for v in (M, dt, 2.0, t, lam)) + f" {n} " + " ".join(bits(v) for v in series[:n].reshape(-1)))
        tr = frontend.Tracer(3, 3, 2.0, fn, initial=np.zeros((3, 3)), decay=lam)
        tr.M[1, 1] = M
        tr.add_source([4], series[:n])
        st = np.zeros((3, 3, 4))                                           # dry, level ground: every cell is a copy case
        tr.apply(st, np.zeros((3, 3)), dt, t)
        want.append(bits(tr.M[1, 1]))
    assert probe(lines) == want


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_a_set_of_tracers_is_that_many_tracers():
    """TracerSet of three species against three Tracer objects, each on a loop of its own: twelve iterations with rain, the inflow
    and sources on species 0 and 2; decay on species 1 and 2."""
    decay = (0.0, 0.25, 3.0)
    M0 = planes()
    st, bed, man = TT.traced_scene()
    fn = TT.functions("f64")
    ts = frontend.TracerSet(ROWS, COLS, DX, fn, initial=M0, decay=decay)
    ts.add_source(0, TT.SOURCE["cells"], TT.SOURCE["series"])
    ts.add_source(2, SOURCE_2["cells"], SOURCE_2["series"])
    loop = TT.TracedLoop(st, bed, man, ts, boundaries=[("uniform", T.RAIN), ("cell", T.INFLOW)])
    loop.step(12)
    assert len(ts) == 3 and ts.iterations == 12 and ts.M.shape == (3, ROWS, COLS)
    for s in range(3):
        tr = frontend.Tracer(ROWS, COLS, DX, fn, initial=M0[s], decay=decay[s])
        if s == 0:
            tr.add_source(TT.SOURCE["cells"], TT.SOURCE["series"])
        if s == 2:
            tr.add_source(SOURCE_2["cells"], SOURCE_2["series"])
        own = TT.TracedLoop(st, bed, man, tr, boundaries=[("uniform", T.RAIN), ("cell", T.INFLOW)])
        own.step(12)
        assert np.array_equal(own.download(), loop.download()) and own.scalars() == loop.scalars()
        assert np.array_equal(tr.M, ts.M[s]) and np.array_equal(tr.M, ts[s].M), s
        assert tr.branch_totals() == ts[s].branch_totals()
        assert (tr.branch_totals()["decayed"] > 0) == (decay[s] > 0)
    assert ts[1].M.any() == False and not np.array_equal(ts.M[2], M0[2])        # zeros stay zeros; the others moved
    totals = ts.branch_totals()
    assert all(totals[name] > 0 for name in ("ring", "moved", "source", "decayed", "e_pos", "w_neg")), totals


def test_a_decaying_tracer_without_decay_is_the_tracer():
    st, bed, man = TT.traced_scene()
    a = frontend.Tracer(ROWS, COLS, DX, TT.functions("f64"), initial=TT.blob())
    b = frontend.Tracer(ROWS, COLS, DX, TT.functions("f64"), initial=TT.blob(), decay=0.0)
    c = frontend.Tracer(ROWS, COLS, DX, TT.functions("f64"), initial=TT.blob(), decay=0.5)
    for tr in (a, b, c):
        TT.TracedLoop(st, bed, man, tr, boundaries=[("cell", T.INFLOW)]).step(4)
    assert np.array_equal(a.M, b.M) and b.branch_totals()["decayed"] == 0
    assert c.M.sum() < a.M.sum() and c.branch_totals()["decayed"] == 4 * ROWS * COLS


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_enable_set_rejects_every_argument_error(probe):
    b = lambda *v: " ".join(bits(x) for x in v)
    who = "bad hp_tracer_enable_set: "
    cases = [
        (f"E 0 2 2 {b(0.0, 1.5)} 3 6 {b(0.0, 1.0, 2.5, 0.0, 0.0, 7.0)}", "ok"),
        ("E 0 1 0 3 0", "ok"),
        ("E 0 8 0 3 0", "ok"),
        ("E null", who + "desc == NULL"),
        ("E 16 2 0 3 0", "bad hp_tracer_set_desc_t size mismatch (ABI)"),
        ("E 0 0 0 3 0", who + "species outside 1..8"),
        ("E 0 9 0 3 0", who + "species outside 1..8"),
        (f"E 0 2 2 {b(0.0, np.nan)} 3 0", who + "species 1: the decay rate must be finite and >= 0"),
        (f"E 0 2 2 {b(-1e-300, 1.0)} 3 0", who + "species 0: the decay rate must be finite and >= 0"),
        (f"E 0 3 3 {b(0.0, 1.0, np.inf)} 3 0", who + "species 2: the decay rate must be finite and >= 0"),
        (f"E 0 2 0 3 6 {b(0.0, 1.0, 2.5, 0.0, -1.0, np.nan)}", who + "species 1, cell 1: initial must be finite and >= 0"),
        (f"E 0 2 0 3 6 {b(0.0, 1.0, np.inf, 0.0, 1.0, 1.0)}", who + "species 0, cell 2: initial must be finite and >= 0"),
    ]
    assert probe([c for c, _ in cases]) == [w for _, w in cases]
    fn = TT.functions("f64")
    for kw, what in ((dict(species=0), "1..8"), (dict(species=9), "1..8"), (dict(decay=[0.0, -1.0]), "species 1: the decay rate"),
                     (dict(decay=[np.nan]), "species 0: the decay rate"), (dict(initial=np.array([[[0.0, 1.0], [1.0, 1.0]], [[0.0, 1.0], [-1.0, 1.0]]])), "species 1: cell 2"),
                     (dict(species=2, decay=[0.0]), "one number of species")):
        with pytest.raises(ValueError, match=what):
            frontend.TracerSet(2, 2, 1.0, fn, **kw)


def test_add_source_to_rejects_every_argument_error(probe):
    s = lambda *pairs: f"{len(pairs)} " + " ".join(bits(v) for p in pairs for v in p)
    good = s((0.0, 1.0), (10.0, 2.0))
    who = "bad hp_tracer_add_source_to: "
    cases = [                                                              # an 8 x 6 grid: the keys of species 1 start at 48
        (f"A 0 3 8 6 0 0 2 9 10 {good}", "ok 9 10"),
        (f"A 1 3 8 6 0 0 2 9 10 {good}", "ok 57 58"),
        (f"A 1 3 8 6 2 9 10 1 2 9 10 {good}", "ok 9 10 57 58"),                 # the same cells in another species: accepted
        (f"A 2 3 8 6 4 9 10 57 58 2 2 9 10 {good}", "ok 9 10 57 58 105 106"),
        (f"A 1 3 8 6 2 57 58 1 2 10 9 {good}", who + "cell 9 is listed twice (another source has it)"),
        (f"A 1 3 8 6 0 0 3 9 10 9 {good}", who + "cell 9 is listed twice"),
        (f"A 3 3 8 6 0 0 2 9 10 {good}", who + "species 3 of a tracer of 3"),
        (f"A 1 1 8 6 0 0 2 9 10 {good}", who + "species 1 of a tracer of 1"),
        (f"A 1 3 8 6 0 0 0 {good}", who + "cells / series == NULL"),
        (f"A 1 3 8 6 0 0 2 9 48 {good}", who + "cell 48 lies outside the grid"),
        (f"A 1 3 8 6 0 0 2 9 16 {good}", who + "cell 16 lies on the grid's edge ring"),
        (f"A 1 3 8 6 0 0 2 9 10 {s((0.0, 1.0), (0.0, 2.0))}", who + "series entry 1: times must be finite and strictly increasing"),
        (f"A 2 3 8 6 1 11 64 2 9 10 {good}", who + "more than 64 sources"),         # the limit holds over the whole set
        (f"A 2 3 8 6 1 11 63 2 9 10 {good}", "ok 11 105 106"),
    ]
    assert probe([c for c, _ in cases]) == [w for _, w in cases]
    ts = frontend.TracerSet(6, 8, 1.0, TT.functions("f64"), species=2)
    ts.add_source(0, [9, 10], [(0.0, 1.0)])
    ts.add_source(1, [9, 10], [(0.0, 1.0)])
    for species, cells, what in ((1, [10], "listed twice"), (2, [11], "species 2 of a tracer of 2"), (0, [16], "edge ring")):
        with pytest.raises(ValueError, match=what):
            ts.add_source(species, cells, [(0.0, 1.0)])


# 5 ---------------------------------------------------------------------------------------------------------------------
MODEL_XML = """<?xml version="1.0"?>
<configuration><metadata><name>tracer set</name></metadata>
<simulation>
  <parameter name="duration" value="2.0"/><parameter name="outputFrequency" value="1.0"/>
  <domainSet><domain type="cartesian" deviceNumber="1">
    <data sourceDir="in" targetDir="out">
      <dataSource type="raster" value="structure,dem" source="dem.asc"/>
      <dataSource type="constant" value="depth" source="1.0"/>
      <dataSource type="constant" value="manningCoefficient" source="0.03"/>
      <tracerSpecies name="river" source="m0.asc"/>
      <tracerSpecies name="sewage" decay="0.25"/>
      <tracerSource species="river" mapFile="cells_a.csv" source="rate_a.csv"/>
      <tracerSource species="sewage" mapFile="cells_b.csv" source="rate_b.csv"/>
      <dataTarget type="raster" value="depth" format="ASC" target="depth_%t.asc"/>
      <dataTarget type="raster" value="tracer" species="river" format="ASC" target="tracer_%t.asc"/>
      <dataTarget type="raster" value="concentration" species="river" format="ASC" target="conc_%t.asc"/>
      <dataTarget type="raster" value="tracer" species="sewage" format="ASC" target="tracer_%s_%t.asc"/>
      <dataTarget type="raster" value="concentration" species="sewage" format="ASC" target="sewage_conc_%t.asc"/>
    </data>
    <scheme name="godunov"><parameter name="courantNumber" value="0.5"/></scheme>
    <boundaryConditions sourceDir="in">
      <domainEdge edge="north" treatment="closed"/><domainEdge edge="south" treatment="closed"/>
      <domainEdge edge="east" treatment="closed"/><domainEdge edge="west" treatment="closed"/>
    </boundaryConditions>
  </domain></domainSet>
</simulation></configuration>
"""
SOURCE_A = dict(cells=[(3, 3), (4, 3)], series=[(0.0, 1.0 / 3.0), (2.0, 1.0)])
SOURCE_B = dict(cells=[(4, 3), (30, 20)], series=[(0.0, 2.0)])
MODEL_COLS, MODEL_ROWS = 40, 32


def write_model(tmp_path, xml=MODEL_XML):
    os.makedirs(tmp_path / "in", exist_ok=True)
    frontend.write_raster(str(tmp_path / "in" / "dem.asc"), np.zeros((MODEL_ROWS, MODEL_COLS)), 2.0)
    m0 = np.zeros((MODEL_ROWS, MODEL_COLS))
    m0[5:8, 6:10] = 1.5
    frontend.write_raster(str(tmp_path / "in" / "m0.asc"), m0, 2.0)
    frontend.write_tracer_source_csv(str(tmp_path / "in" / "cells_a.csv"), str(tmp_path / "in" / "rate_a.csv"), SOURCE_A["cells"], SOURCE_A["series"])
    frontend.write_tracer_source_csv(str(tmp_path / "in" / "cells_b.csv"), str(tmp_path / "in" / "rate_b.csv"), SOURCE_B["cells"], SOURCE_B["series"])
    path = tmp_path / "model.xml"
    path.write_text(xml)
    return str(path), m0


def test_the_model_file_elements_parse(tmp_path):
    xml, _ = write_model(tmp_path)
    cfg = frontend.parse_configuration(xml)
    assert cfg.tracer_species == [dict(name="river", decay=0.0, initial="m0.asc"), dict(name="sewage", decay=0.25, initial=None)]
    assert [s["species"] for s in cfg.tracer_sources] == ["river", "sewage"] and cfg.tracer_sources[1]["cells"] == SOURCE_B["cells"]
    assert [what for what, _ in cfg.targets] == ["depth", "tracer", "concentration", "tracer", "concentration"]
    assert cfg.target_species == [None, "river", "river", "sewage", "sewage"]


class Sim(oracle.OracleSim):
    """The oracle with a tracer set that does not move: what Model hands to the engine, and what it writes."""

    def tracer_enable(self, initial=None):
        self.single = True

    def tracer_enable_set(self, initial=None, decay=None, species=None):
        self.m, self.decay, self.set_sources = np.array(initial), list(decay), []

    def tracer_add_source(self, cells, series, species=0):
        self.set_sources.append((species, list(cells), np.array(series)))

    def tracer_read(self, row0=0, nrows=None, species=0):
        return self.m[species].copy()


def make_sim(cfg, cols, rows, res):
    return Sim(cols, rows, dx=res, scheme=cfg.scheme, precision=cfg.precision, end_time=cfg.duration)


def test_model_hands_its_tracer_set_to_the_engine(tmp_path):
    from hipims_mi.model import Model
    xml, m0 = write_model(tmp_path)
    m = Model(xml, make_sim=make_sim, output_format=".npy")
    assert m.tracer is None and m.tracer_set["names"] == ["river", "sewage"] and m.sim.decay == [0.0, 0.25]
    assert np.array_equal(m.sim.m[0], m0) and not m.sim.m[1].any()
    assert [(s, c) for s, c, _ in m.sim.set_sources] == [(0, SOURCE_A["cells"]), (1, SOURCE_B["cells"])]
    m.sim.m[1, 20, 30] = 0.75
    m.run()
    out = tmp_path / "out"
    assert np.array_equal(np.load(out / "tracer_river_2.npy"), m0) and np.array_equal(np.load(out / "tracer_sewage_2.npy"), m.sim.m[1])
    assert np.array_equal(np.load(out / "conc_river_2.npy"), frontend.tracer_concentration(m0, m.sim.download(), m.bed))
    assert np.array_equal(np.load(out / "sewage_conc_2.npy"), frontend.tracer_concentration(m.sim.m[1], m.sim.download(), m.bed))
    assert np.load(out / "sewage_conc_2.npy")[20, 30] == 0.75
    # Model(tracers=...) on a file without the elements
    bare = "\n".join(l for l in MODEL_XML.splitlines() if "<tracerS" not in l and "species=" not in l)
    xml2, _ = write_model(tmp_path / "bare", bare)
    spec = [dict(name="a", initial=m0, decay=1.0, sources=[dict(cells=[(5, 5)], series=[(0.0, 2.0)])]), dict(name="b")]
    m = Model(xml2, make_sim=make_sim, tracers=spec, output_format=".npy")
    assert m.tracer_set["names"] == ["a", "b"] and m.sim.decay == [1.0, 0.0] and m.sim.set_sources[0][:2] == (0, [(5, 5)])
    # both forms are refused, in the arguments and in the file; so is an engine without a set, and a target without its species
    with pytest.raises(ValueError, match="one or the other"):
        Model(xml2, make_sim=make_sim, tracers=spec, tracer=dict(initial=None, sources=[]))
    with pytest.raises(ValueError, match="one or the other"):
        Model(xml, make_sim=make_sim, tracer=dict(initial=None, sources=[]))
    both = write_model(tmp_path / "both", MODEL_XML.replace('<tracerSpecies name="river"', '<tracerSource mapFile="cells_a.csv" source="rate_a.csv"/>\n<tracerSpecies name="river"'))[0]
    with pytest.raises(ValueError, match="one or the other"):
        Model(both, make_sim=make_sim)
    with pytest.raises(NotImplementedError):
        Model(xml, make_sim=lambda cfg, cols, rows, res: oracle.OracleSim(cols, rows, dx=res, scheme=cfg.scheme, precision=cfg.precision, end_time=cfg.duration))
    unnamed = write_model(tmp_path / "unnamed", MODEL_XML.replace('value="tracer" species="river"', 'value="tracer"'))[0]
    with pytest.raises(ValueError, match="must name one of its species"):
        Model(unnamed, make_sim=make_sim)
    stray = write_model(tmp_path / "stray", MODEL_XML.replace('<tracerSource species="sewage"', '<tracerSource species="rain"'))[0]
    with pytest.raises(ValueError, match="'rain'"):
        Model(stray, make_sim=make_sim)
