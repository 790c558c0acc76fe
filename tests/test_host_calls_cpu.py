"""The host-call fuzz without a GPU (tests/host_calls.py): the generator is deterministic, every operation kind and each of the four
call patterns behind the round-6 findings occurs, and the oracle's own run of the linearised sequences stays finite on at least
95 % of each leg's seeds -- the cap on what test_gpu_host_calls.py may leave uncompared.  The oracle runs are shared by the tests of
this module."""
import collections
import functools

import numpy as np
import pytest

import host_calls as hc


@functools.lru_cache(maxsize=None)
def sequences(leg):
    return [hc.make_sequence(hc.SEED_BASE[leg] + i, leg) for i in range(hc.SEEDS_PER_LEG)]


@functools.lru_cache(maxsize=None)
def oracle_runs(leg):
    return [hc.run_on_oracle(s) if s["oracle_ok"] else None for s in sequences(leg)]


def test_the_generator_is_deterministic():
    for leg in hc.LEGS:
        for seed in (hc.SEED_BASE[leg], hc.SEED_BASE[leg] + 57):
            a, b = hc.make_sequence(seed, leg), hc.make_sequence(seed, leg)
            assert hc.describe(a) == hc.describe(b) and a["patterns"] == b["patterns"]
            assert np.array_equal(a["cfg"]["st"], b["cfg"]["st"]) and np.array_equal(a["cfg"]["bed"], b["cfg"]["bed"])
            for x, y in zip(a["ops"], b["ops"]):
                assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))
    s = hc.make_sequence(hc.SEED_BASE["strict"] + 3, "strict")
    assert hc.digest(hc.run_on_oracle(s)) == hc.digest(hc.run_on_oracle(s))


@pytest.mark.parametrize("leg", hc.LEGS)
def test_sizes_and_lengths_stay_inside_the_bounds(leg):
    for s in sequences(leg):
        c = s["cfg"]
        assert c["cols"] in hc.COLS and c["rows"] in hc.ROWS and s["iterations"] <= hc.MAX_ITERATIONS
        assert 8 <= len([o for o in s["ops"]]) <= 23                       # 8-20 drawn, up to two boundaries in front, the final download
        assert c["dynamic"] or not any(o[0] in hc.BOUNDARY_OPS for o in s["ops"])
        assert leg == "fast" or s["oracle_ok"]
        assert leg != "spec" or c["precision"] == "f64"
    schemes = collections.Counter(s["cfg"]["scheme"] for s in sequences(leg))
    assert 0.55 <= schemes[hc.GODUNOV] / hc.SEEDS_PER_LEG <= 0.85 and schemes[hc.MUSCL] and schemes[hc.INERTIAL]
    assert {s["cfg"]["terrain"] for s in sequences(leg)} == {"rough", "dam"}
    assert {s["cfg"]["friction"] for s in sequences(leg)} == {True, False} and {s["cfg"]["dynamic"] for s in sequences(leg)} == {True, False}


def test_every_operation_kind_and_every_pattern_occurs():
    kinds, patterns = collections.Counter(), collections.Counter()
    for leg in hc.LEGS:
        leg_kinds = collections.Counter(hc.op_name(o) for s in sequences(leg) for o in s["ops"])
        kinds.update(leg_kinds)
        for s in sequences(leg):
            patterns.update({k: v for k, v in s["patterns"].items() if v})
        wanted = [k for k in hc.OP_KINDS if leg == "fast" or k not in hc.ORACLE_LESS]
        assert all(leg_kinds[k] > 0 for k in wanted), (leg, [k for k in wanted if not leg_kinds[k]])
    print("operations: " + ", ".join(f"{k} {kinds[k]}" for k in hc.OP_KINDS))
    print("patterns: " + ", ".join(f"{k} {patterns[k]}" for k in hc.PATTERNS))
    assert set(kinds) == set(hc.OP_KINDS)
    assert all(patterns[k] >= 3 for k in hc.PATTERNS), patterns


@pytest.mark.parametrize("leg", hc.LEGS)
def test_the_oracle_stays_finite_on_95_percent_of_the_seeds(leg):
    runs = [r for r in oracle_runs(leg) if r is not None]
    finite = sum(r["finite"] for r in runs)
    rebuilt = sum(r["rebuilds"] > 0 for r in runs)
    print(f"{leg}: oracle runs {len(runs)} of {hc.SEEDS_PER_LEG} seeds, finite {finite} ({100.0 * finite / len(runs):.1f} %), with a restore {rebuilt}")
    assert len(runs) >= (hc.SEEDS_PER_LEG if leg != "fast" else hc.SEEDS_PER_LEG // 3)
    assert finite >= 0.95 * len(runs)
    assert rebuilt >= 10


def test_the_fp32_oracle_can_measure_most_fp32_sequences():
    """test_gpu_host_calls.py holds a FAST fp32 run to the fp32 oracle at 1e-4 m only where the oracle's own rounding error (against
    itself in fp64, host_calls.reference_error) stays below a tenth of that.  The comparison must not wither: at least half of the
    leg's fp32 sequences the oracle can follow, and at least five of them, are measurable that way."""
    cases = [(s, r) for s, r in zip(sequences("fast"), oracle_runs("fast")) if r is not None and r["finite"] and s["cfg"]["precision"] == "f32"]
    errors = [hc.reference_error(s, r) for s, r in cases]
    usable = sum(e < hc.REFERENCE_ERROR_SHARE * 1e-4 for e in errors)
    print(f"fast, fp32: {usable} of {len(cases)} sequences have an oracle within {hc.REFERENCE_ERROR_SHARE * 1e-4:.0e} m of itself in fp64; the others: "
          + ", ".join(f"seed {s['cfg']['seed']} {e:.2e} m" for (s, _), e in zip(cases, errors) if e >= hc.REFERENCE_ERROR_SHARE * 1e-4))
    assert usable >= 5 and 2 * usable >= len(cases)
    assert all(hc.reference_error(s, r) == 0.0 for s, r in zip(sequences("fast")[:10], oracle_runs("fast")[:10]) if r is not None and s["cfg"]["precision"] == "f64")


def test_a_restore_brings_the_twin_back_to_the_checkpoint():
    """The twin's own claim, on the oracle alone: run, save, wander off (another target, a bed change), restore, finish == a straight
    run on which the bed change arrives at the restore point."""
    s = hc.make_sequence(hc.SEED_BASE["strict"], "strict")
    s = dict(s, ops=[("batch", 7), ("save",), ("target", 0.05), ("batch", 9), ("bed", 0.02), ("split", 2), ("restore",), ("batch", 8), ("download",)])
    a = hc.run_on_oracle(s)
    # (the straight run: the bed op's update_timestep is a scalar change and is rolled back with the checkpoint -- emulate by hand)
    twin = hc.OracleTwin(s["cfg"])
    twin.upload(s["cfg"]["st"], s["cfg"]["bed"], s["cfg"]["man"]); twin.set_target(1e9)
    twin.step_batch(7)
    twin.upload(bed=a["bed"])
    twin.step_batch(8)
    assert np.array_equal(twin.download(), a["points"][0]) and twin.scalars() == a["scalars"]
