"""The moving bed without a GPU: the shared C++ definition of the fraction and the new bed (csrc/hp_bed.hpp, in a stand-alone
program: tests/bed_probe.cpp) against the NumPy restatement (frontend.BedShapes) bit for bit, BedShapes.apply on hand-made arrays,
the entry points' argument checks through the built library, the model file's <bedShape> and a run on the oracle engine.
Bit patterns and exact comparisons: the only tolerance is the one rounding a kept depth is allowed."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import hipims_mi as hp
import oracle
from conftest import ROOT
from hipims_mi import frontend
from test_abi import declared_functions

CSRC = os.path.join(ROOT, "hipims-ocl_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))

bits = lambda v: struct.pack(">d", float(v)).hex()
from_bits = lambda s: struct.unpack(">d", bytes.fromhex(s))[0]
ulp_up = lambda v: float(np.nextafter(v, np.inf))
ulp_down = lambda v: float(np.nextafter(v, -np.inf))

SERIES = {
    1: [(5.0, 0.25)],
    2: [(2.0, 0.0), (12.0, 1.0)],
    7: [(0.1, 0.0), (0.7, 0.3), (1.0 / 3.0 + 1.0, 0.3), (2.5, 1.0), (3.1, 0.4), (7.0, 0.0), (1e3, 1.0)],      # non-monotone: a gate reopens
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bed") / "bed_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "bed_probe.cpp")])

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


def times_of(series):
    knots = [t for t, _ in series]
    ts = [knots[0] - 1.0, knots[-1] + 1.0, -1e300, 1e300, 0.0]
    for k in knots:
        ts += [k, ulp_up(k), ulp_down(k)]
    for a, b in zip(knots, knots[1:]):
        ts += [a + (b - a) / 3.0, a + (b - a) * 0.5, a + (b - a) * 0.9371]
    return ts


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_the_shared_definition_needs_no_hip():
    host = open(os.path.join(CSRC, "hp_bed.hpp")).read().split("#ifdef __HIPCC__\n#include")[0]
    code = "\n".join(l.split("//")[0] for l in host.splitlines())
    assert "bed_fraction" in code and "bed_level" in code and "bed_round" in code
    assert "#include <hip" not in code and "__global__" not in code and "hp_math" not in code


@pytest.mark.parametrize("entries", [1, 2, 7])
def test_fraction_equals_the_restatement_bit_for_bit(probe, entries):
    series = SERIES[entries]
    ts = times_of(series)
    flat = " ".join(bits(v) for pair in series for v in pair)
    got = probe([f"F {entries} {bits(t)} {flat}" for t in ts])
    for t, g in zip(ts, got):
        want = frontend.BedShapes.series_fraction(series, t)
        assert g == bits(want), (t, from_bits(g), want)
        assert 0.0 <= want <= 1.0
    # the rules themselves, on values that need no arithmetic
    f = lambda t: frontend.BedShapes.series_fraction(series, t)
    assert f(series[0][0]) == series[0][1] and f(series[0][0] - 1.0) == series[0][1] and f(ulp_down(series[0][0])) == series[0][1]
    assert f(series[-1][0]) == series[-1][1] and f(series[-1][0] + 1.0) == series[-1][1] and f(ulp_up(series[-1][0])) == series[-1][1]
    for t, fr in series:
        assert f(t) == fr                                                          # on a knot: the knot's fraction
    if entries == 2:
        assert f(7.0) == 0.5 and f(4.5) == 0.25 and f(2.0) == 0.0 and f(12.0) == 1.0          # f exactly 0 and exactly 1
    if entries == 7:
        assert f(2.8) < 1.0 and f(5.0) < f(3.1)                                    # falling again


def test_new_bed_equals_the_restatement_bit_for_bit(probe):
    rng = np.random.default_rng(5)
    # a pair for which base + (target - base) is not the target: found here, and the property asserted
    pair = None
    for _ in range(10000):
        b, t = float(rng.uniform(-50, 50)), float(rng.uniform(-50, 50))
        if b + (t - b) != t:
            pair = (b, t)
            break
    assert pair is not None and pair[0] + (pair[1] - pair[0]) != pair[1]
    cases = [(pair[0], pair[1], f) for f in (0.0, 1.0, 1.0 - 2.0 ** -53, 0.5, 2.0 ** -1074, -0.0)]
    cases += [(float(rng.uniform(-100, 100)), float(rng.uniform(-100, 100)), float(f)) for f in rng.random(200)]
    cases += [(5.0, 0.5, f) for f in (0.0, 1.0, 0.3, 1.0 / 3.0, 0.999999)] + [(0.1, 0.1, 0.7), (-9999.0, 9999.0, 0.5)]
    got = probe([f"L {bits(b)} {bits(t)} {bits(f)}" for b, t, f in cases])
    for (b, t, f), line in zip(cases, got):
        g64, g32 = line.split()
        want = float(frontend.BedShapes.level(np.array([b]), np.array([t]), f)[0])
        assert g64 == bits(want), (b, t, f)
        assert g32 == bits(np.float32(want)), (b, t, f)                             # rounded once
    level = lambda b, t, f: float(frontend.BedShapes.level(np.array([b]), np.array([t]), f)[0])
    assert level(pair[0], pair[1], 1.0) == pair[1]                                 # f >= 1: the target itself
    assert level(pair[0], pair[1], 0.0) == pair[0] and level(pair[0], pair[1], -0.0) == pair[0]
    assert from_bits(got[1].split()[0]) == pair[1] and from_bits(got[0].split()[0]) == pair[0]


# 2 ---------------------------------------------------------------------------------------------------------------------
def hand_made(dtype):
    """5 rows x 6 columns: a flat bed at 1 m under 0.75 m of water, a wall cell, a disabled cell."""
    bed = np.full((5, 6), 1.0, dtype)
    state = np.zeros((5, 6, 4), dtype)
    state[..., 0] = 1.75
    state[..., 1] = 1.75
    state[..., 2] = 0.125
    state[..., 3] = -0.25
    bed[2, 3] = 9999.9                                 # a wall cell
    state[3, 1, 1] = -9999.0                           # a disabled cell
    state[1, 4, 1] = 9.0                               # a maximum from earlier
    return state, bed


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_apply_on_hand_made_arrays(dtype):
    state, bed = hand_made(dtype)
    shapes = frontend.BedShapes(5, 6)
    moved = [(1, 1), (2, 1), (4, 1), (2, 2)]           # (x, y)
    shapes.add(moved + [(3, 2), (1, 3)], [0.3, 0.1, 2.6, 1.0 / 3.0, 0.5, 0.5], [(1.0, 0.0), (3.0, 1.0)], bed=bed)
    shapes.add([5 * 6 - 1], 4.0, [(0.0, 0.0), (10.0, 0.0)], bed=bed)              # a shape that never moves
    with pytest.raises(ValueError, match="listed twice"):
        shapes.add([(1, 1)], 0.0, [(0.0, 0.0)])
    with pytest.raises(ValueError, match="fraction"):
        shapes.add([(0, 0)], 0.0, [(0.0, 1.5)])
    with pytest.raises(ValueError, match="increasing"):
        shapes.add([(0, 0)], 0.0, [(0.0, 0.5), (0.0, 0.6)])
    assert shapes.fraction(2.0) == [0.5, 0.0]
    s0, b0 = state.copy(), bed.copy()
    assert shapes.apply(state, bed, 0.5) == 0 and np.array_equal(state, s0) and np.array_equal(bed, b0)      # before the series: nothing moves
    changed = shapes.apply(state, bed, 2.0)
    assert changed == 4
    eps = np.finfo(dtype).eps
    for x, y in moved:
        target = {(1, 1): 0.3, (2, 1): 0.1, (4, 1): 2.6, (2, 2): 1.0 / 3.0}[(x, y)]
        want_bed = dtype(1.0 + 0.5 * (target - 1.0))
        assert bed[y, x] == want_bed                                                # rounded once, from fp64
        depth0 = float(s0[y, x, 0]) - float(b0[y, x])
        depth1 = float(state[y, x, 0]) - float(bed[y, x])
        assert abs(depth1 - depth0) <= eps * max(1.0, abs(float(state[y, x, 0])))   # the depth, to one rounding
        assert state[y, x, 1] >= state[y, x, 0]
        assert np.array_equal(state[y, x, 2:], s0[y, x, 2:])                        # Qx, Qy as they are
    assert state[1, 4, 1] == 9.0                                                    # the larger maximum stays
    assert state[1, 1, 1] == s0[1, 1, 1] and state[1, 1, 0] < s0[1, 1, 0]            # a level that fell keeps its maximum
    untouched = np.ones((5, 6), bool)
    for x, y in moved:
        untouched[y, x] = False
    assert np.array_equal(state[untouched], s0[untouched]) and np.array_equal(bed[untouched], b0[untouched])      # wall, disabled, unmoved, unlisted
    assert bed[2, 3] == dtype(9999.9) and state[3, 1, 1] == -9999.0 and bed[3, 1] == 1.0
    assert shapes.apply(state, bed, 2.0) == 0                                       # the same time again: b1 == b0 everywhere
    assert shapes.apply(state, bed, 99.0) == 4 and bed[1, 1] == dtype(0.3) and bed[2, 2] == dtype(1.0 / 3.0)      # f >= 1: the targets, rounded once
    if dtype is np.float32:
        # one rounding: the fp64 result rounded, not a result formed in fp32
        st32, bd32 = hand_made(np.float32)
        sh = frontend.BedShapes(5, 6)
        sh.add([(2, 2)], 1.0 / 3.0, [(0.0, 0.0), (3.0, 1.0)], bed=bd32)
        sh.apply(st32, bd32, 1.0)
        f = frontend.BedShapes.series_fraction([(0.0, 0.0), (3.0, 1.0)], 1.0)
        b1 = np.float32(1.0 + f * (1.0 / 3.0 - 1.0))
        assert bd32[2, 2] == b1 and st32[2, 2, 0] == np.float32(float(b1) + (float(np.float32(1.75)) - 1.0))


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    lib = hp.load_library()
    for name in ("hp_bed_shape_add", "hp_bed_shapes_clear", "hp_bed_apply", "hp_bed_info"):
        assert name in declared_functions() and hasattr(lib, name) and name in hp.EXPORTS
    assert C.sizeof(hp.BedShapeDesc) == 40 and C.sizeof(hp.BedInfo) == 48
    from hipims_mi import strips
    for name in ("bed_shape_add", "bed_shapes_clear", "bed_apply", "bed_info"):
        assert callable(getattr(hp.Domain, name))
    for name in ("bed_shape_add", "bed_shapes_clear", "bed_apply", "gather_bed"):
        assert callable(getattr(strips.StripRunner, name))


def test_argument_errors_are_invalid_before_any_device_call():
    """With a NULL domain: every check that does not need the domain comes first and names what is wrong; the rest is "null
    domain".  No device is touched (this machine may have none)."""
    lib = hp.load_library()

    def add(cells, target, series, size=None, null=None):
        c, t, s = np.array(cells, np.uint64), np.array(target, np.float64), np.array(series, np.float64).reshape(-1, 2)
        desc = hp.BedShapeDesc(C.sizeof(hp.BedShapeDesc) if size is None else size, len(s), c.size, c.ctypes.data_as(C.POINTER(C.c_uint64)),
                               t.ctypes.data_as(C.POINTER(C.c_double)), s.ctypes.data_as(C.POINTER(C.c_double)))
        if null:
            setattr(desc, null, None)
        return lib.hp_bed_shape_add(None, C.byref(desc)), lib.hp_last_error().decode()

    good = ([3, 4, 5], [0.5, 0.5, 0.5], [(2.0, 0.0), (12.0, 1.0)])
    assert add(*good) == (-1, "null domain")                                        # a NULL domain, everything else in order
    cases = [
        (dict(size=8), "size mismatch"),
        (dict(null="cells"), "== NULL"), (dict(null="target"), "== NULL"), (dict(null="series"), "== NULL"),
        (dict(cells=[3, 4, 3]), "cell 3 is listed twice"),                          # a repeated cell: named
        (dict(series=[(2.0, 0.0), (12.0, 1.5)]), "fraction outside [0, 1]"),
        (dict(series=[(2.0, 0.0), (12.0, float("nan"))]), "fraction outside [0, 1]"),
        (dict(series=[(2.0, 0.0), (2.0, 1.0)]), "strictly increasing"),             # equal times
        (dict(series=[(2.0, 0.0), (1.0, 1.0)]), "strictly increasing"),
        (dict(series=[(float("inf"), 0.0)]), "finite"),
        (dict(target=[0.5, float("nan"), 0.5]), "target 1"),
        (dict(target=[0.5, 0.5, 9999.5]), "target 2"),
        (dict(series=np.zeros((0, 2))), "series_entries outside 1..4096"),
        (dict(series=np.stack([np.arange(4097.0), np.zeros(4097)], axis=1)), "series_entries outside 1..4096"),
    ]
    for change, message in cases:
        kw = {k: change.pop(k) for k in ("size", "null") if k in change}
        args = dict(zip(("cells", "target", "series"), good), **change)
        rc, text = add(args["cells"], args["target"], args["series"], **kw)
        assert rc == -1 and message in text, (message, text)
    assert lib.hp_bed_shape_add(None, None) == -1 and b"desc == NULL" in lib.hp_last_error()
    info = hp.BedInfo(C.sizeof(hp.BedInfo))
    for rc in (lib.hp_bed_apply(None), lib.hp_bed_shapes_clear(None), lib.hp_bed_info(None, C.byref(info))):
        assert rc == -1 and b"null domain" in lib.hp_last_error()
    assert lib.hp_bed_info(None, None) == -1 and b"out == NULL" in lib.hp_last_error()
    info.struct_size = 4
    assert lib.hp_bed_info(None, C.byref(info)) == -1 and b"size mismatch" in lib.hp_last_error()


def block_image(shapes, cols, row_lo, row_hi, esize):
    """The device block of the shapes' lists, restated from the layout comment of csrc/hp_bed.hpp:
    [cells: n x 8 | target: n x 8 | series: pairs x 16 | base: n elements, padded to 8 | series_off: (shapes + 1) x 4, padded to 8 |
    shape_of: n, at least one byte].  `shapes`: (global ids, targets, series) each; the strip keeps the ids of its rows, as local ids.
    Returns the seven figures of the layout, the bytes (base zero: the device fills it) and the regions' sizes before padding."""
    cells, target, shape_of, series, series_off = [], [], [], [], [0]
    for s, (ids, tg, sr) in enumerate(shapes):
        for c, t in zip(ids, tg):
            if row_lo <= c // cols < row_hi:
                cells.append(c - row_lo * cols)
                target.append(t)
                shape_of.append(s)
        series += [v for pair in sr for v in pair]
        series_off.append(len(series) // 2)
    n, pad8 = len(cells), lambda b: b + b"\0" * (-len(b) % 8)
    regions = [np.array(cells, "<u8").tobytes(), np.array(target, "<f8").tobytes(), np.array(series, "<f8").tobytes(), bytes(n * esize),
               np.array(series_off, "<u4").tobytes(), np.array(shape_of, "u1").tobytes() if n else b"\0"]
    padded = regions[:3] + [pad8(regions[3]), pad8(regions[4]), regions[5]]
    offsets = [sum(len(r) for r in padded[:k]) for k in range(7)]
    return offsets, b"".join(padded), [len(r) for r in regions]


@pytest.mark.parametrize("esize", [4, 8])
def test_layout_and_image_of_the_device_block_equal_the_restatement(probe, esize):
    """validate_bed_shape, bed_layout and bed_image through the probe: a first shape, a second on top of it, cell counts that are no
    multiple of 8 (5 and 5 + 6: both paddings are met, base's with 4-byte elements, series_off's with two shapes), and strips that
    hold none of a shape's cells."""
    cols, grows = 10, 12
    first = ([53, 54, 55, 64, 97], [0.5, -1.25, 3.0, 1.0 / 3.0, 9999.0], [(2.0, 0.0), (12.0, 1.0)])
    second = ([61, 62, 63, 71, 72, 108], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6], [(0.0, 0.0), (1.5, 0.75), (4.0, 0.25)])
    flat = lambda s: f"{len(s[0])} {len(s[2])} " + " ".join(str(c) for c in s[0]) + " " + " ".join(bits(t) for t in s[1]) + " " + \
        " ".join(bits(v) for pair in s[2] for v in pair)
    strips = [(0, 12), (5, 8), (0, 3), (7, 9), (9, 12)]              # whole grid; part of both; none of either (n == 0); none of the first; one cell of each
    cases = [(shapes, lo, hi) for lo, hi in strips for shapes in ([first], [first, second])]
    got = probe([f"B {esize} {cols} {grows} {lo} {hi} {len(shapes)} " + " ".join(flat(s) for s in shapes) for shapes, lo, hi in cases])
    images = {}
    for (shapes, lo, hi), line in zip(cases, got):
        *figures, image = line.split()
        offsets, want, sizes = block_image(shapes, cols, lo, hi, esize)
        assert [int(v) for v in figures] == offsets, (lo, hi, len(shapes))
        assert bytes.fromhex(image) == want and len(want) == offsets[6], (lo, hi, len(shapes))
        for k in range(6):                                                          # disjoint, in order, 8-aligned
            assert offsets[k] % 8 == 0 and offsets[k] + sizes[k] <= offsets[k + 1] < offsets[k] + sizes[k] + 8
        images[(len(shapes), lo, hi)] = (offsets, bytes.fromhex(image), sizes)
    n_of = lambda key: images[key][2][0] // 8
    assert n_of((1, 0, 12)) == 5 and n_of((2, 0, 12)) == 11 and n_of((2, 0, 3)) == 0 and n_of((1, 7, 9)) == 0 and n_of((2, 7, 9)) == 2
    assert n_of((1, 9, 12)) == 1 and n_of((2, 9, 12)) == 2
    assert images[(2, 0, 3)][0][6] == images[(2, 0, 3)][0][5] + 1                   # n == 0: one shape_of byte all the same
    for lo, hi in strips:                                                           # the first shape's entries, carried over unchanged
        (o1, b1, s1), (o2, b2, _) = images[(1, lo, hi)], images[(2, lo, hi)]
        for k, size in ((0, s1[0]), (1, s1[1]), (2, s1[2]), (4, s1[4]), (5, s1[0] // 8)):
            assert b2[o2[k]:o2[k] + size] == b1[o1[k]:o1[k] + size], (lo, hi, k)
        assert b2[o2[4] + 8:o2[4] + 12] == struct.pack("<I", 5)                     # ... and the second's series behind the first's
    # the checks in front of it, in the entry point's order: a cell of the new shape that an earlier one has
    again = ([10, 97], [0.0, 0.0], [(0.0, 1.0)])
    beyond = ([cols * grows], [0.0], [(0.0, 1.0)])
    refused = probe([f"B {esize} {cols} {grows} 0 12 2 {flat(first)} {flat(again)}", f"B {esize} {cols} {grows} 0 12 1 {flat(beyond)}"])
    assert refused[0] == "! hp_bed_shape_add: cell 97 is listed twice (another shape has it)"
    assert refused[1] == "! hp_bed_shape_add: cell 120 lies outside the grid"


# 4 ---------------------------------------------------------------------------------------------------------------------
XML ="""<?xml version="1.0"?>
<configuration>
  <metadata><name>reservoir behind a wall</name></metadata>
  <simulation>
    <parameter name="duration" value="{duration}" />
    <parameter name="outputFrequency" value="{frequency}" />
    <parameter name="floatingPointPrecision" value="double" />
    <domainSet>
      <domain type="cartesian" deviceNumber="1">
        <data sourceDir="topography/" targetDir="output/">
          <dataSource type="constant" value="manningCoefficient" source="0.030" />
          <dataSource type="raster" value="structure,dem" source="dem.asc" />
          <dataSource type="raster" value="depth" source="depth.asc" />
          <dataTarget type="raster" value="depth" target="depth_%t.npy" />
          {shapes}
        </data>
        <scheme name="Godunov">
          <parameter name="courantNumber" value="0.50" />
          <parameter name="frictionEffects" value="yes" />
        </scheme>
        <boundaryConditions sourceDir="./">
          <domainEdge edge="north" treatment="closed" /><domainEdge edge="south" treatment="closed" />
          <domainEdge edge="east" treatment="closed" /><domainEdge edge="west" treatment="closed" />
        </boundaryConditions>
      </domain>
    </domainSet>
  </simulation>
</configuration>
"""
COLS, ROWS, WALL = 48, 40, (22, 23)                   # the wall's two columns


def reservoir(tmpdir, in_file, duration=12, frequency=2):
    root = str(tmpdir)
    os.makedirs(os.path.join(root, "topography"), exist_ok=True)
    dem = np.zeros((ROWS, COLS))
    dem[:, WALL[0]:WALL[1] + 1] = 3.0
    depth = np.zeros((ROWS, COLS))
    depth[:, :WALL[0]] = 2.0
    # (0.5 m cells: the CFL timestep stays below the reference's 0.1 s early limit, so every sync point is met by a clipped step)
    frontend.write_raster(os.path.join(root, "topography", "dem.asc"), dem, 0.5)
    frontend.write_raster(os.path.join(root, "topography", "depth.asc"), depth, 0.5)
    cells = [(x, y) for y in range(14, 26) for x in WALL]
    series = [(4.0, 0.0), (6.0, 0.5), (8.0, 1.0)]
    with open(os.path.join(root, "topography", "cells.csv"), "w") as f:
        f.write("x,y,target\n" + "".join(f"{x},{y},0.25\n" for x, y in cells))
    with open(os.path.join(root, "topography", "progress.csv"), "w") as f:
        f.write("time,fraction\n" + "".join(f"{t},{fr}\n" for t, fr in series))
    element = '<bedShape name="breach" mapFile="cells.csv" source="progress.csv"/>' if in_file else ""
    xml = os.path.join(root, "model.xml")
    open(xml, "w").write(XML.format(duration=duration, frequency=frequency, shapes=element))
    return xml, cells, series


def _oracle_sim(cfg, cols, rows, res):
    return oracle.OracleSim(cols, rows, dx=res, scheme=cfg.scheme, very_small=cfg.dry_threshold, courant=cfg.courant,
                            end_time=cfg.duration, friction=cfg.friction, threads=4)


def test_parse_configuration_reads_bed_shapes(tmp_path):
    xml, cells, series = reservoir(tmp_path / "a", True)
    cfg = frontend.parse_configuration(xml)
    assert len(cfg.bed_shapes) == 1
    b = cfg.bed_shapes[0]
    assert b["name"] == "breach" and b["cells"] == cells and np.array_equal(b["target"], np.full(len(cells), 0.25))
    assert np.array_equal(b["series"], np.array(series))
    assert frontend.parse_configuration(reservoir(tmp_path / "b", False)[0]).bed_shapes == []


@pytest.mark.parametrize("in_file", [True, False])
def test_a_breach_on_the_oracle_engine(tmp_path, in_file):
    """A 48 x 40 reservoir behind a wall that fails between 4 s and 8 s: dry downstream until the series starts, wet at the end,
    the bed at the shape's cells at its targets.  (The oracle engine has no bed_apply: this is the host path, frontend.BedShapes.)"""
    from hipims_mi.model import Model
    xml, cells, series = reservoir(tmp_path, in_file)
    lines = []
    kw = {} if in_file else dict(bed_shapes=[dict(cells=cells, target=0.25, series=series)])
    m = Model(xml, make_sim=_oracle_sim, output_format=None, log=lines.append, **kw)
    m.scheme.automatic_queue = False
    m.scheme.queue_addition_size = 8
    assert not m.device_beds and m.host_beds is not None and m.bed_applies == 1     # once after the initial upload
    outs = m.run()
    times = [t for t, _ in outs]
    assert times == [2.0, 4.0, 6.0, 8.0, 10.0, 12.0]
    downstream = np.s_[1:-1, WALL[1] + 1:-1]
    before = [o["depth"] for t, o in outs if t <= series[0][0]][-1]                 # the last output before the series starts
    assert float(before[downstream].max()) <= 1e-8
    last = outs[-1][1]["depth"]
    assert float(last[downstream].max()) > 0.05 and int((last[downstream] > 1e-3).sum()) > 100
    xs, ys = np.array(cells)[:, 0], np.array(cells)[:, 1]
    assert np.array_equal(m.bed[ys, xs], np.full(len(cells), 0.25))                 # the targets, at the end
    assert np.array_equal(m._bed_real[ys, xs], np.full(len(cells), 0.25))
    wall_left = np.ones(ROWS, bool)
    wall_left[14:26] = False
    wall_left[[0, -1]] = False
    assert (m.bed[wall_left][:, WALL[0]] == 3.0).all()                              # the rest of the wall stands
    assert 1 < m.bed_applies < 2 + m.scheme.iterations // 8                         # not behind every batch: only while a shape can move
    assert any(f"{m.bed_applies} bed applies" in l for l in lines if "Output files written" in l)
    volume = lambda depth: float(np.where(depth > 0.0, depth, 0.0).sum())           # (NODATA on the walls)
    assert abs(volume(last) - volume(outs[0][1]["depth"])) < 1e-6 * volume(last)    # the depth is kept where the bed moves
    m.close()
