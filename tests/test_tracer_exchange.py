"""A tracer species' exchange with the bed without a GPU: the shared C++ definition of step 7 and its cube root (csrc/hp_tracer.hpp,
csrc/hp_crmath.h, in a stand-alone program: tests/tracer_exchange_probe.cpp) against the NumPy restatement
(frontend.Tracer(exchange=...), frontend.cbrt_exact) bit for bit, the host checks of hp_tracer_set_exchange, the restatement's physics
on the scene of tests/test_links.py, and the model file's attributes."""
import ctypes as C
import math
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
INF = float("inf")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tracer_exchange") / "tracer_exchange_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "tracer_exchange_probe.cpp")])

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


def test_abi_additions():
    lib = hp.load_library()
    for name in ("hp_tracer_set_exchange", "hp_tracer_deposit_read", "hp_tracer_deposit_write", "hp_tracer_exchange_info"):
        assert name in declared_functions() and hasattr(lib, name) and name in hp.EXPORTS
    assert lib.hp_abi_version() == 2 and C.sizeof(hp.TracerExchangeDesc) == 48
    for name in ("tracer_set_exchange", "tracer_deposit_read", "tracer_deposit_write", "tracer_exchange_info"):
        assert hasattr(hp.Domain, name)
    # argument errors come before any device call: a NULL domain is one, with or without a GPU
    assert lib.hp_tracer_set_exchange(None, None) == -1 and lib.hp_tracer_exchange_info(None, None, None) == -1
    assert lib.hp_tracer_deposit_read(None, 0, None, 0, 0) == -1 and lib.hp_tracer_deposit_write(None, 0, None, 0, 0) == -1
    host = open(os.path.join(CSRC, "hp_tracer.hpp")).read().split("#ifdef __HIPCC__\n#include")[0]
    assert "tracer_exchange(" in host and "validate_tracer_exchange" in host


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_the_cube_root_equals_exact_integer_arithmetic_in_every_bit(probe):
    rng = np.random.default_rng(20291)
    xs = list(np.ldexp(rng.uniform(1.0, 2.0, 3000), rng.integers(-40, 21, 3000)))
    for k in list(range(1, 200)) + [1 << 17, 208063, (1 << 17) + 1]:          # perfect cubes (exact in a double) and their two neighbours
        c = float(k) ** 3
        assert int(c) == k ** 3
        xs += [c, np.nextafter(c, 0.0), np.nextafter(c, INF)]
    for k in (3, 5, 7, 11, 1001):                                             # ... and cubes of binary fractions
        c = (k / 1024.0) ** 3
        xs += [c, np.nextafter(c, 0.0), np.nextafter(c, INF)]
    xs += [1e-10, np.nextafter(1e-10, INF), 1.0, 8.0, 0.001]
    out = probe(["C " + bits(x) for x in xs])
    for x, got in zip(xs, out):
        assert got == bits(frontend.cbrt_exact(x)), (x, from_bits(got), frontend.cbrt_exact(x))
    assert frontend.cbrt_exact(27.0) == 3.0 and frontend.cbrt_exact(2.0 ** -30) == 2.0 ** -10 and frontend.cbrt_exact(3.0) ** 3 != 3.0
    assert np.array_equal(frontend.cbrt_exact_array(np.array([[8.0, 27.0], [8.0, 1e-3]])), np.array([[2.0, 3.0], [2.0, frontend.cbrt_exact(1e-3)]]))
    for bad in (0.0, -1.0, INF, float("nan")):
        with pytest.raises(ValueError):
            frontend.cbrt_exact(bad)


# 2 ---------------------------------------------------------------------------------------------------------------------
def tau_of(h, qx, qy, n):
    return float(frontend.Tracer.shear(h, qx, qy, n))


def exchange_cases():
    """(M, D, h, qx, qy, n, dt, settling, tau_deposit, tau_erode, erodibility): random ones, then the edges."""
    rng = np.random.default_rng(20292)
    n_random = 4000
    cases = []
    for _ in range(n_random):
        h = float(rng.choice([10.0 ** rng.uniform(-9.5, 1.0), 1e-10, 9.9e-11, 0.0, -1e-3], p=[0.9, 0.025, 0.025, 0.025, 0.025]))
        tcd = float(rng.choice([10.0 ** rng.uniform(-3, 2), INF], p=[0.85, 0.15]))
        tce = float(rng.choice([tcd, tcd * (1.0 + 10.0 ** rng.uniform(-3, 1)), INF], p=[0.2, 0.6, 0.2]))
        cases.append((float(rng.uniform(0, 5) * (rng.random() > 0.1)), float(rng.uniform(0, 2) * (rng.random() > 0.2)), h,
                      float(rng.normal() * 10.0 ** rng.uniform(-4, 1)), float(rng.normal() * 10.0 ** rng.uniform(-4, 1)),
                      float(rng.choice([0.03, 0.0, np.float64(np.float32(0.035)), rng.uniform(0.01, 0.1)])), float(10.0 ** rng.uniform(-5, 1)),
                      float(rng.choice([0.0, 10.0 ** rng.uniform(-5, -1)])), tcd, tce, float(rng.choice([0.0, 10.0 ** rng.uniform(-6, 0)]))))
    # tau just below, at and above each threshold: the thresholds are set from the water's own tau
    h, qx, qy, n = 0.75, 0.6, -0.3, 0.03
    tau = tau_of(h, qx, qy, n)
    below, above = float(np.nextafter(tau, 0.0)), float(np.nextafter(tau, INF))
    for tcd in (below, tau, above):
        for tce in (t for t in (below, tau, above, 2.0 * tau, INF) if t >= tcd):
            cases.append((1.5, 0.25, h, qx, qy, n, 0.1, 1e-3, tcd, tce, 1e-2))
    cases += [
        (1.5, 0.25, h, qx, qy, n, 0.1, 1e-3, INF, INF, 1e-2),                  # tau_deposit = +inf: probability 1
        (1.5, 0.25, h, 0.0, 0.0, n, 0.1, 1e-3, INF, INF, 0.0),                 # still water settles
        (1.5, 0.25, h, qx, qy, n, 0.1, 1e-3, tau / 4, INF, 1e-2),              # tau_erode = +inf: never erodes
        (1.5, 1e-9, h, qx, qy, n, 0.1, 0.0, tau / 4, tau / 2, 1.0),            # ero > D: D goes to exactly 0
        (1.5, 0.25, h, qx, qy, n, 1e300, 0.0, tau / 4, tau / 2, 1.0),          # ... by a huge dt
        (0.0, 0.25, h, 0.0, 0.0, n, 0.1, 1e-3, INF, INF, 1e-2),                # M'' <= 0: nothing to deposit
        (-0.5, 0.25, h, 0.0, 0.0, n, 0.1, 1e-3, INF, INF, 1e-2),
        (1.5, 0.25, 1e-10, qx, qy, n, 0.1, 1e-3, INF, INF, 1e-2),              # h at the threshold: nothing happens
        (1.5, 0.25, float(np.nextafter(1e-10, INF)), 1e-12, 0.0, n, 0.1, 1e-3, INF, INF, 1e-2),   # ... and just above it
        (1.5, 0.25, float(np.nextafter(1e-10, INF)), 1e-3, 1e-3, n, 0.1, 1e-3, 1.0, 2.0, 1e-2),  # a huge tau from a thin film
        (1.5, 0.25, h, qx, qy, 0.0, 0.1, 1e-3, 0.5, 1.0, 1e-2),                # n = 0: no shear stress, deposits
        (1.5, 0.25, h, qx, qy, n, 1e-300, 1e-3, INF, INF, 1e-2),               # dt tiny
        (1.5, 0.25, h, qx, qy, n, 1e300, 1e-3, INF, INF, 1e-2),                # dt huge: everything settles, nothing overshoots
        (1.5, 0.25, h, float("nan"), qy, n, 0.1, 1e-3, INF, INF, 1e-2),         # NaN discharge: both comparisons fail
        (1.5, 0.25, h, qx, float("nan"), n, 0.1, 1e-3, 1.0, 2.0, 1e-2),
        (1.5, 0.0, h, qx, qy, n, 0.1, 0.0, tau / 4, tau / 2, 1.0),             # nothing lies on the ground
    ]
    return cases, n_random


def test_step_7_equals_the_restatement_bit_for_bit(probe):
    cases, n_random = exchange_cases()
    out = probe(["X " + " ".join(bits(v) for v in c) for c in cases])
    seen = {"deposited": 0, "eroded": 0, "nothing": 0, "clipped": 0, "shallow": 0, "nan": 0}
    for c, got in zip(cases, out):
        M, D, h, qx, qy, n, dt, ws, tcd, tce, E = c
        q = frontend.Tracer.exchange_params(dict(settling=ws, tau_deposit=tcd, tau_erode=tce, erodibility=E))
        M1, D1, dep, ero = frontend.Tracer.exchange_step(M, D, h, qx, qy, n, dt, q)
        assert got == bits(M1) + " " + bits(D1), (c, [from_bits(g) for g in got.split()], float(M1), float(D1))
        assert not (dep and ero)
        seen["deposited"] += bool(dep)
        seen["eroded"] += bool(ero)
        seen["nothing"] += not (dep or ero)
        seen["clipped"] += bool(ero) and float(D1) == 0.0
        seen["shallow"] += not h > 1e-10
        seen["nan"] += bool(np.isnan(qx) or np.isnan(qy))
        if not (dep or ero):
            assert got == bits(M) + " " + bits(D)
        if dep:
            assert 0.0 <= float(M1) <= M and float(D1) >= D                   # implicit Euler never overshoots zero
        if ero:
            assert 0.0 <= float(D1) <= D and float(M1) >= M
    assert all(v > 0 for v in seen.values()), seen
    assert seen["deposited"] > 300 and seen["eroded"] > 100, seen
    # the threshold cases one by one: deposition needs tau < tau_deposit, erosion tau > tau_erode, both strictly
    h, qx, qy, n = 0.75, 0.6, -0.3, 0.03
    tau = tau_of(h, qx, qy, n)
    q = lambda tcd, tce: frontend.Tracer.exchange_params(dict(settling=1e-3, tau_deposit=tcd, tau_erode=tce, erodibility=1e-2))
    step = lambda tcd, tce: tuple(bool(v) for v in frontend.Tracer.exchange_step(1.5, 0.25, h, qx, qy, n, 0.1, q(tcd, tce))[2:])
    below, above = float(np.nextafter(tau, 0.0)), float(np.nextafter(tau, INF))
    assert step(above, INF) == (True, False) and step(tau, INF) == (False, False) and step(below, INF) == (False, False)
    assert step(below, below) == (False, True) and step(below, tau) == (False, False) and step(tau, above) == (False, False)
    assert math.isclose(tau, 9810.0 * 0.03 ** 2 * ((0.6 / 0.75) ** 2 + (0.3 / 0.75) ** 2) / 0.75 ** (1.0 / 3.0), rel_tol=1e-14)


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_set_exchange_rejects_every_argument_error(probe):
    b = lambda *v: " ".join(bits(x) for x in v)
    who = "bad hp_tracer_set_exchange: "
    good = b(1e-3, 0.5, 1.0, 1e-2)
    cases = [
        (f"V 0 1 2 {good} 3 3 {b(0.0, 1.0, 2.5)}", "ok"),
        (f"V 0 0 1 {b(0.0, INF, INF, 0.0)} 3 0", "ok"),
        (f"V 0 0 1 {b(1e-3, 0.5, 0.5, 0.0)} 3 0", "ok"),
        ("V null", who + "desc == NULL"),
        (f"V 40 0 1 {good} 3 0", "bad hp_tracer_exchange_desc_t size mismatch (ABI)"),
        (f"V 0 2 2 {good} 3 0", who + "species 2 of a tracer of 2"),
        (f"V 0 1 1 {good} 3 0", who + "species 1 of a tracer of 1"),
        (f"V 0 0 1 {b(-1e-300, 0.5, 1.0, 1e-2)} 3 0", who + "settling must be finite and >= 0"),
        (f"V 0 0 1 {b(INF, 0.5, 1.0, 1e-2)} 3 0", who + "settling must be finite and >= 0"),
        (f"V 0 0 1 {b(np.nan, 0.5, 1.0, 1e-2)} 3 0", who + "settling must be finite and >= 0"),
        (f"V 0 0 1 {b(1e-3, 0.0, 1.0, 1e-2)} 3 0", who + "tau_deposit must be > 0 (+inf allowed)"),
        (f"V 0 0 1 {b(1e-3, -1.0, 1.0, 1e-2)} 3 0", who + "tau_deposit must be > 0 (+inf allowed)"),
        (f"V 0 0 1 {b(1e-3, np.nan, 1.0, 1e-2)} 3 0", who + "tau_deposit must be > 0 (+inf allowed)"),
        (f"V 0 0 1 {b(1e-3, 0.5, 0.25, 1e-2)} 3 0", who + "tau_erode must be >= tau_deposit (+inf allowed)"),
        (f"V 0 0 1 {b(1e-3, INF, 1.0, 1e-2)} 3 0", who + "tau_erode must be >= tau_deposit (+inf allowed)"),
        (f"V 0 0 1 {b(1e-3, 0.5, np.nan, 1e-2)} 3 0", who + "tau_erode must be >= tau_deposit (+inf allowed)"),
        (f"V 0 0 1 {b(1e-3, 0.5, 1.0, -1.0)} 3 0", who + "erodibility must be finite and >= 0"),
        (f"V 0 0 1 {b(1e-3, 0.5, 1.0, INF)} 3 0", who + "erodibility must be finite and >= 0"),
        (f"V 0 0 1 {good} 3 3 {b(0.0, -1.0, np.nan)}", who + "cell 1: deposit_initial must be finite and >= 0"),
        (f"V 0 0 1 {good} 3 3 {b(0.0, 1.0, INF)}", who + "cell 2: deposit_initial must be finite and >= 0"),
        # the header's order: the species before the fields, the fields in their order, the raster last
        (f"V 0 3 2 {b(-1.0, 0.0, -1.0, -1.0)} 3 3 {b(-1.0, 0.0, 0.0)}", who + "species 3 of a tracer of 2"),
        (f"V 0 0 2 {b(-1.0, 0.0, -1.0, -1.0)} 3 3 {b(-1.0, 0.0, 0.0)}", who + "settling must be finite and >= 0"),
        (f"V 0 0 2 {b(0.0, 0.0, -1.0, -1.0)} 3 3 {b(-1.0, 0.0, 0.0)}", who + "tau_deposit must be > 0 (+inf allowed)"),
        (f"V 0 0 2 {b(0.0, 1.0, 0.5, -1.0)} 3 3 {b(-1.0, 0.0, 0.0)}", who + "tau_erode must be >= tau_deposit (+inf allowed)"),
        (f"V 0 0 2 {b(0.0, 1.0, 1.0, -1.0)} 3 3 {b(-1.0, 0.0, 0.0)}", who + "erodibility must be finite and >= 0"),
        (f"V 0 0 2 {b(0.0, 1.0, 1.0, 0.0)} 3 3 {b(-1.0, 0.0, 0.0)}", who + "cell 0: deposit_initial must be finite and >= 0"),
    ]
    assert probe([c for c, _ in cases]) == [w for _, w in cases]
    fn = TT.functions("f64")
    for kw, what in ((dict(exchange=dict(settling=-1.0)), "settling must be finite and >= 0"), (dict(exchange=dict(settling=INF)), "settling must be finite"),
                     (dict(exchange=dict(tau_deposit=0.0)), "tau_deposit must be > 0"), (dict(exchange=dict(tau_deposit=np.nan)), "tau_deposit must be > 0"),
                     (dict(exchange=dict(tau_deposit=1.0, tau_erode=0.5)), "tau_erode must be >= tau_deposit"),
                     (dict(exchange=dict(tau_deposit=INF, tau_erode=1.0)), "tau_erode must be >= tau_deposit"),
                     (dict(exchange=dict(erodibility=-1.0)), "erodibility must be finite and >= 0"), (dict(exchange=dict(erodibility=np.nan)), "erodibility must be finite"),
                     (dict(exchange=dict(speed=1.0)), "no parameter 'speed'"),
                     (dict(exchange=dict(settling=1e-3), deposit=[[0.0, 1.0], [-1.0, np.nan]]), "cell 2: deposit_initial must be finite and >= 0"),
                     (dict(exchange=dict(settling=1e-3), deposit=np.zeros((3, 2))), "must be")):
        with pytest.raises(ValueError, match=what):
            frontend.Tracer(2, 2, 1.0, fn, **kw)
    with pytest.raises(ValueError, match="species 1: tau_erode"):
        frontend.TracerSet(2, 2, 1.0, fn, species=2, exchange=[None, dict(tau_deposit=2.0, tau_erode=1.0)])
    with pytest.raises(ValueError, match="one number of species"):
        frontend.TracerSet(2, 2, 1.0, fn, species=2, exchange=[None])


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_mass_and_deposit_together_keep_the_closed_domain_mass():
    """The closed-domain scene of tests/test_tracer.py with a species that deposits and erodes, lambda = 0: fsum(M) + fsum(D) moves by
    no more than that test's bound, cells * iterations * 2^-52 * largest, `largest` the largest M or D met in the run.  Exchange adds
    two roundings a cell and iteration (the M3 quotient with its difference, or the two sides of the eroded mass), which the bound's
    half-weight count has room for: measured here, the drift stays far inside it."""
    iterations = 30
    st, bed, man = TT.traced_scene(enable_all=True)
    m0, d0 = TT.blob(), np.full((ROWS, COLS), 0.125)                        # (a deposit everywhere: the fast water is not where the blob is)
    tr = frontend.Tracer(ROWS, COLS, DX, TT.functions("f64"), initial=m0, deposit=d0, manning=man,
                         exchange=dict(settling=2e-2, tau_deposit=1e-5, tau_erode=1e-4, erodibility=5e-3))   # (the scene's shear stress reaches 2e-3 N/m2)
    loop = TT.TracedLoop(st, bed, man, tr, boundaries=[("uniform", T.RAIN), ("cell", T.INFLOW)])
    largest = float(max(m0.max(), d0.max()))
    for _ in range(iterations):
        loop.step(1)
        largest = max(largest, float(np.abs(tr.M).max()), float(np.abs(tr.D).max()))
    before = math.fsum(list(m0.reshape(-1)) + list(d0.reshape(-1)))
    after = math.fsum(list(tr.M.reshape(-1)) + list(tr.D.reshape(-1)))
    bound = ROWS * COLS * iterations * 2.0 ** -52 * largest
    totals = tr.branch_totals()
    print(f"sum(M) + sum(D): {before!r} -> {after!r}, change {after - before:.3e}, bound {bound:.3e}, largest {largest!r}, "
          f"deposited {totals['deposited']}, eroded {totals['eroded']}")
    assert totals["deposited"] > 1000 and totals["eroded"] > 0, totals
    assert not np.array_equal(tr.D, d0) and (tr.D >= 0).all() and (tr.M >= 0).all()
    assert abs(after - before) <= bound


def test_still_water_only_settles():
    """tau_deposit = +inf, erodibility = 0, water at rest: M falls and D rises monotonically at every cell, M never goes below 0."""
    st, bed, man = TT.traced_scene(enable_all=True)
    st[..., 2:] = 0.0
    wet = st[..., 0] - bed > 1e-3
    st[..., 0] = st[..., 1] = np.where(wet, st[..., 0][wet].max(), st[..., 0])  # one level: nothing moves the water
    m0 = TT.blob()
    tr = frontend.Tracer(ROWS, COLS, DX, TT.functions("f64"), initial=m0, manning=man, exchange=dict(settling=5e-2, erodibility=0.0))
    loop = TT.TracedLoop(st, bed, man, tr)
    M, D, total = tr.M.copy(), tr.D.copy(), []
    for _ in range(8):
        loop.step(1)
        assert (tr.D >= D).all() and (tr.M >= 0).all()
        total.append((math.fsum(tr.M.reshape(-1)), math.fsum(tr.D.reshape(-1))))
        M, D = tr.M.copy(), tr.D.copy()
    assert all(a[0] > b[0] and a[1] < b[1] for a, b in zip(total, total[1:])), total
    assert tr.branch_totals()["deposited"] > 0 and tr.branch_totals()["eroded"] == 0
    assert abs(total[-1][0] + total[-1][1] - math.fsum(m0.reshape(-1))) <= ROWS * COLS * 8 * 2.0 ** -52 * float(m0.max())


def test_zero_parameters_are_no_exchange():
    st, bed, man = TT.traced_scene()
    d0 = np.where(TT.blob() > 0.5, 0.125, 0.0)
    a = frontend.Tracer(ROWS, COLS, DX, TT.functions("f64"), initial=TT.blob(), decay=0.25)
    b = frontend.Tracer(ROWS, COLS, DX, TT.functions("f64"), initial=TT.blob(), decay=0.25, deposit=d0, manning=man,
                        exchange=dict(settling=0.0, tau_deposit=0.5, tau_erode=1.0, erodibility=0.0))
    for tr in (a, b):
        TT.TracedLoop(st, bed, man, tr, boundaries=[("cell", T.INFLOW)]).step(5)
    assert np.array_equal(a.M, b.M) and np.array_equal(b.D, d0) and not a.D.any()
    assert b.branch_totals()["deposited"] == 0 == b.branch_totals()["eroded"]
    ts = frontend.TracerSet(ROWS, COLS, DX, TT.functions("f64"), initial=[TT.blob(), TT.blob()], exchange=[None, dict(settling=1e-2)], manning=man)
    TT.TracedLoop(st, bed, man, ts, boundaries=[("cell", T.INFLOW)]).step(3)
    assert ts.D.shape == (2, ROWS, COLS) and not ts.D[0].any() and ts.D[1].any() and ts.branch_totals()["deposited"] > 0


# 5 ---------------------------------------------------------------------------------------------------------------------
MODEL_XML = """<?xml version="1.0"?>
<configuration><metadata><name>tracer exchange</name></metadata>
<simulation>
  <parameter name="duration" value="2.0"/><parameter name="outputFrequency" value="1.0"/>
  <domainSet><domain type="cartesian" deviceNumber="1">
    <data sourceDir="in" targetDir="out">
      <dataSource type="raster" value="structure,dem" source="dem.asc"/>
      <dataSource type="constant" value="depth" source="1.0"/>
      <dataSource type="constant" value="manningCoefficient" source="0.03"/>
      <tracerSpecies name="silt" source="m0.asc" settling="0.001" tauDeposit="0.08" tauErode="0.25" erodibility="0.0002" deposit="d0.asc"/>
      <tracerSpecies name="dye" decay="0.25"/>
      <dataTarget type="raster" value="depth" format="ASC" target="depth_%t.asc"/>
      <dataTarget type="raster" value="tracer" species="silt" format="ASC" target="tracer_%t.asc"/>
      <dataTarget type="raster" value="deposit" species="silt" format="ASC" target="deposit_%t.asc"/>
    </data>
    <scheme name="godunov"><parameter name="courantNumber" value="0.5"/></scheme>
    <boundaryConditions sourceDir="in">
      <domainEdge edge="north" treatment="closed"/><domainEdge edge="south" treatment="closed"/>
      <domainEdge edge="east" treatment="closed"/><domainEdge edge="west" treatment="closed"/>
    </boundaryConditions>
  </domain></domainSet>
</simulation></configuration>
"""
MODEL_COLS, MODEL_ROWS = 24, 16


def write_model(tmp_path, xml=MODEL_XML):
    os.makedirs(tmp_path / "in", exist_ok=True)
    frontend.write_raster(str(tmp_path / "in" / "dem.asc"), np.zeros((MODEL_ROWS, MODEL_COLS)), 2.0)
    m0, d0 = np.zeros((MODEL_ROWS, MODEL_COLS)), np.zeros((MODEL_ROWS, MODEL_COLS))
    m0[5:8, 6:10] = 1.5
    d0[9:12, 3:20] = 0.25
    frontend.write_raster(str(tmp_path / "in" / "m0.asc"), m0, 2.0)
    frontend.write_raster(str(tmp_path / "in" / "d0.asc"), d0, 2.0)
    path = tmp_path / "model.xml"
    path.write_text(xml)
    return str(path), m0, d0


def test_the_model_file_attributes_parse(tmp_path):
    xml, _, _ = write_model(tmp_path)
    cfg = frontend.parse_configuration(xml)
    assert cfg.tracer_species == [dict(name="silt", decay=0.0, initial="m0.asc", deposit="d0.asc",
                                       exchange=dict(settling=0.001, tau_deposit=0.08, tau_erode=0.25, erodibility=0.0002)),
                                  dict(name="dye", decay=0.25, initial=None)]
    assert [what for what, _ in cfg.targets] == ["depth", "tracer", "deposit"] and cfg.target_species == [None, "silt", "silt"]


class SetSim(oracle.OracleSim):
    """The oracle with a tracer set that does not move: an engine from before the exchange."""

    def tracer_enable_set(self, initial=None, decay=None, species=None):
        self.m, self.decay, self.exchange = np.array(initial), list(decay), {}
        self.d = np.zeros_like(self.m)

    def tracer_add_source(self, cells, series, species=0):
        raise AssertionError("the model has no source")

    def tracer_read(self, row0=0, nrows=None, species=0):
        return self.m[species].copy()


class Sim(SetSim):
    """... and with a deposit that neither settles nor erodes: what Model hands to the engine, and what it writes."""

    def tracer_set_exchange(self, species, settling=0.0, tau_deposit=INF, tau_erode=INF, erodibility=0.0, deposit=None):
        self.exchange[species] = dict(settling=settling, tau_deposit=tau_deposit, tau_erode=tau_erode, erodibility=erodibility)
        if deposit is not None:
            self.d[species] = deposit

    def tracer_deposit_read(self, species=0, row0=0, nrows=None):
        return self.d[species].copy()


def make_sim(cfg, cols, rows, res):
    return Sim(cols, rows, dx=res, scheme=cfg.scheme, precision=cfg.precision, end_time=cfg.duration)


def test_model_hands_the_exchange_to_the_engine(tmp_path):
    from hipims_mi.model import Model
    xml, m0, d0 = write_model(tmp_path)
    m = Model(xml, make_sim=make_sim, output_format=".npy")
    assert m.tracer is None and m.tracer_set["names"] == ["silt", "dye"]
    assert m.sim.exchange == {0: dict(settling=0.001, tau_deposit=0.08, tau_erode=0.25, erodibility=0.0002)}
    assert np.array_equal(m.sim.d[0], d0) and not m.sim.d[1].any() and m.tracer_set["exchange"][1] is None
    m.sim.d[0, 2, 3] = 0.75
    m.run()
    out = tmp_path / "out"
    assert np.array_equal(np.load(out / "deposit_silt_2.npy"), m.sim.d[0]) and np.load(out / "deposit_silt_1.npy")[2, 3] == 0.75
    assert np.array_equal(np.load(out / "tracer_silt_2.npy"), m0)
    assert [sorted(k for k in o if isinstance(k, tuple)) for _, o in m.outputs][-1] == [("deposit", "silt"), ("tracer", "silt")]
    # Model(tracers=...) on a file without the elements: a single species with an exchange is a set of one
    bare = "\n".join(l for l in MODEL_XML.splitlines() if "<tracerS" not in l and "species=" not in l)
    xml2, _, _ = write_model(tmp_path / "bare", bare)
    m = Model(xml2, make_sim=make_sim, tracers=[dict(name="mud", initial=m0, exchange=dict(settling=0.5), deposit=d0)], output_format=".npy")
    assert m.tracer is None and m.tracer_set["names"] == ["mud"] and np.array_equal(m.sim.d[0], d0)
    assert m.sim.exchange == {0: dict(settling=0.5, tau_deposit=INF, tau_erode=INF, erodibility=0.0)}
    # refused: a bad value, a deposit target of a species that does not exchange or that nobody declares, an engine without the call
    with pytest.raises(ValueError, match="tau_erode must be >= tau_deposit"):
        Model(xml2, make_sim=make_sim, tracers=[dict(name="mud", exchange=dict(tau_deposit=1.0, tau_erode=0.5))])
    for swap in (('value="deposit" species="silt"', 'value="deposit" species="dye"'), ('value="deposit" species="silt"', 'value="deposit" species="sand"'),
                 ('value="deposit" species="silt"', 'value="deposit"')):
        other = write_model(tmp_path / ("swap" + str(abs(hash(swap)))), MODEL_XML.replace(*swap))[0]
        with pytest.raises(ValueError, match="a deposit data target must name a species"):
            Model(other, make_sim=make_sim)

    with pytest.raises(NotImplementedError, match="tracer_set_exchange"):
        Model(xml, make_sim=lambda cfg, cols, rows, res: SetSim(cols, rows, dx=res, scheme=cfg.scheme, precision=cfg.precision, end_time=cfg.duration))
