"""The actors' host-call fuzz without a GPU (tests/host_calls_actors.py): the stepwise twin equals the oracle -- checkpoints
included -- on every sequence of the old legs it can run; make_sequence still returns what it returned before the actors came; the
actor sequences are deterministic, keep their rules (disjoint cells, at most MAX_EXTRA more operations, no MUSCL-Hancock), contain
every new operation and every call pattern the fuzz is about; and the twin's own run stays finite on at least 95 % of each leg's
seeds -- the cap on what test_gpu_host_calls_actors.py may leave uncompared.  The twin's runs are shared by the tests of this module."""
import collections
import functools
import hashlib

import numpy as np
import pytest

import host_calls as hc
import host_calls_actors as ha

# SHA-256 over describe(make_sequence(seed, leg)) and the raw bytes of st, bed and man of the 360 seeds of the old legs, computed
# on the commit before the actors' fuzz was added
OLD_SEQUENCES_SHA256 = "8f005751cd8d0081c6ed6cedc845d9a88367c72d48970425b5c100479d8fb45c"


@functools.lru_cache(maxsize=None)
def sequences(leg):
    return [ha.make_actor_sequence(ha.SEED_BASE[leg] + i, leg) for i in range(ha.SEEDS_PER_LEG)]


@functools.lru_cache(maxsize=None)
def twin_runs(leg):
    return [ha.run_on_twin(s) if s["twin_ok"] else None for s in sequences(leg)]


def test_make_sequence_returns_what_it_returned_before():
    h = hashlib.sha256()
    for leg in hc.LEGS:
        for i in range(hc.SEEDS_PER_LEG):
            s = hc.make_sequence(hc.SEED_BASE[leg] + i, leg)
            h.update(hc.describe(s).encode())
            for key in ("st", "bed", "man"):
                h.update(np.ascontiguousarray(s["cfg"][key]).tobytes())
    assert h.hexdigest() == OLD_SEQUENCES_SHA256


@pytest.mark.parametrize("leg", ["strict", "spec"])
def test_the_stepwise_twin_equals_the_oracle_on_the_old_legs(leg):
    """Every oracle_ok sequence of the old `strict` and `spec` legs that is not MUSCL-Hancock: the twin's states at every download
    and its scalars are the oracle's bits.  Save and restore are among the operations, so the twin's direct restatement of the
    checkpoint is held to the replay twin the engine already matches."""
    held = restores = 0
    for i in range(hc.SEEDS_PER_LEG):
        seq = hc.make_sequence(hc.SEED_BASE[leg] + i, leg)
        if not seq["oracle_ok"] or seq["cfg"]["scheme"] == hc.MUSCL:
            continue
        want, got = hc.run_on_oracle(seq), ha.run_on_twin(seq)
        assert hc.digest(got) == hc.digest(want), f"seed {seq['cfg']['seed']}: {hc.describe(seq)}"
        assert np.array_equal(got["bed"], want["bed"])
        held += 1
        restores += any(o[0] == "restore" for o in seq["ops"])
    print(f"{leg}: {held} sequences, {restores} with a restore")
    assert held >= 0.75 * hc.SEEDS_PER_LEG and restores >= 10
    with pytest.raises(NotImplementedError):
        ha.StepTwin(dict(seq["cfg"], scheme=hc.MUSCL))


def test_the_generator_is_deterministic_and_keeps_the_old_operations():
    for leg in ha.LEGS:
        for seed in (ha.SEED_BASE[leg], ha.SEED_BASE[leg] + 41):
            a, b = ha.make_actor_sequence(seed, leg), ha.make_actor_sequence(seed, leg)
            assert ha.describe(a) == ha.describe(b) and a["patterns"] == b["patterns"]
            assert np.array_equal(a["cfg"]["st"], b["cfg"]["st"]) and np.array_equal(a["cfg"]["bed"], b["cfg"]["bed"])
            for x, y in zip(a["ops"], b["ops"]):
                assert len(x) == len(y) and repr(x) == repr(y)
            old = hc.make_sequence(seed, leg)
            kept = [o for o in a["ops"] if o[0] not in ha.ACTOR_KINDS]
            extra_clear = len(kept) - len(old["ops"])            # (an inserted `clear` is the only old kind that is added)
            assert 0 <= extra_clear <= 1 and [hc.op_name(o) for o in kept if o[0] != "clear"] == [hc.op_name(o) for o in old["ops"] if o[0] != "clear"]
    s = sequences("strict")[3]
    assert ha.digest(ha.run_on_twin(s)) == ha.digest(ha.run_on_twin(s))


@pytest.mark.parametrize("leg", ha.LEGS)
def test_the_sequences_keep_their_rules(leg):
    for s in sequences(leg):
        c = s["cfg"]
        old = hc.make_sequence(c["seed"], leg)
        rows, cols = c["rows"], c["cols"]
        assert c["scheme"] in (hc.GODUNOV, hc.INERTIAL) and cols in hc.COLS and rows in hc.ROWS and s["iterations"] <= hc.MAX_ITERATIONS
        assert (c["scheme"] == old["cfg"]["scheme"]) or old["cfg"]["scheme"] == hc.MUSCL
        assert 1 <= len(s["ops"]) - len(old["ops"]) <= ha.MAX_EXTRA and s["ops"][-1] == ("download",)
        assert leg == "fast" or s["twin_ok"]
        patch, shape_cells, ends, groups = ha.bed_patch(rows, cols), [], [], 0
        first_apply = next(i for i, o in enumerate(s["ops"]) if o[0] == "bed_apply")
        assert any(o[0] == "shape" for o in s["ops"][:first_apply])
        for o in s["ops"]:
            if o[0] == "shape":
                cells, target, series = o[1].astype(np.int64), o[2], o[3]
                y, x = cells // cols, cells % cols
                assert 1 <= len(cells) <= 40 and ((y >= 1) & (y < rows - 1) & (x >= 1) & (x < cols - 1)).all() and not patch[y, x].any()
                assert 2 <= len(series) <= 4 and (np.diff(series[:, 0]) > 0).all() and series[0, 0] > 0
                assert ((series[:, 1] >= 0) & (series[:, 1] <= 1)).all()
                base = c["bed"].reshape(-1)[cells].astype(np.float64)
                assert (np.abs(target - base)[np.abs(base) < 9000] <= 0.5 + 1e-12).all() and (np.abs(target) <= 9999).all()
                shape_cells += cells.tolist()
            elif o[0] == "links":
                groups += 1
                assert 1 <= len(o[1]) <= 6
                for l in o[1]:
                    for e in (l["a"], l["b"]):
                        assert 1 <= e // cols < rows - 1 and 1 <= e % cols < cols - 1
                    ends += [l["a"], l["b"]]
        assert len(set(shape_cells)) == len(shape_cells) and len(set(ends)) == len(ends) and groups <= 3


def test_every_new_operation_and_every_pattern_occurs():
    for leg in ha.LEGS:
        kinds = collections.Counter(o[0] for s in sequences(leg) for o in s["ops"])
        patterns = collections.Counter()
        links = [l for s in sequences(leg) for o in s["ops"] if o[0] == "links" for l in o[1]]
        for s in sequences(leg):
            patterns.update({k: v for k, v in s["patterns"].items() if v})
        print(f"{leg}: operations " + ", ".join(f"{k} {kinds[k]}" for k in ha.ACTOR_KINDS + ('clear',)) + "; patterns " +
              ", ".join(f"{k} {patterns[k]}" for k in ha.PATTERNS))
        assert all(kinds[k] > 0 for k in ha.ACTOR_KINDS + ("clear",)), kinds
        assert all(patterns[k] >= 1 for k in ha.LEG_PATTERNS[leg]), (leg, patterns)
        assert all(patterns[k] == 0 for k in ha.PATTERNS if k not in ha.LEG_PATTERNS[leg]), (leg, patterns)
        # all three kinds, a flap valve, an uncapped orifice, a link of no size, an end on a null cell
        assert {l["kind"] for l in links} == {ha.WEIR, ha.ORIFICE, ha.PUMP}
        assert any(l["one_way"] for l in links) and any(l["size"] == 0.0 for l in links)
        assert any(l["kind"] == ha.ORIFICE and l["limit"] == np.inf for l in links)
        null_ends = sum(int(s["cfg"]["st"].reshape(-1, 4)[e, 1] <= -9000) for s in sequences(leg) for o in s["ops"] if o[0] == "links"
                        for l in o[1] for e in (l["a"], l["b"]))
        assert null_ends >= 1
        assert {s["patterns_old"][k] > 0 for s in sequences(leg) for k in hc.PATTERNS} == {True, False}


@pytest.mark.parametrize("leg", ha.LEGS)
def test_the_twin_stays_finite_on_95_percent_of_the_seeds_and_the_actors_act(leg):
    runs = [r for r in twin_runs(leg) if r is not None]
    finite = sum(r["finite"] for r in runs)
    moved = sum(r["changed_total"] > 0 for r in runs)
    flowed = sum(r["links_active"] > 0 or any(int(p[2]["active"].sum()) > 0 for p in r["points"]) for r in runs)
    warned = sum(r["warnings"] > 0 for r in runs)
    print(f"{leg}: twin runs {len(runs)} of {ha.SEEDS_PER_LEG} seeds, finite {finite} ({100.0 * finite / len(runs):.1f} %); an apply moved the bed on "
          f"{moved}, a link moved water on {flowed}, a restore warned on {warned}")
    assert len(runs) >= (ha.SEEDS_PER_LEG if leg != "fast" else ha.SEEDS_PER_LEG // 3)
    assert finite >= 0.95 * len(runs)
    for first in range(0, ha.SEEDS_PER_LEG, ha.CHUNK):               # ... and chunk by chunk, as the GPU tests leave out
        chunk = [r for r in twin_runs(leg)[first:first + ha.CHUNK] if r is not None]
        assert sum(not r["finite"] for r in chunk) <= 0.05 * ha.CHUNK
    assert moved >= len(runs) // 4 and flowed >= len(runs) // 6 and warned >= 1


def test_a_restore_follows_the_header():
    """The twin's checkpoint, rule by rule, on one small scene: state, scalars and phase come back; the bed at the listed cells comes
    back while the shapes are the same and the records while the groups are; a shape or group added since costs one warning each."""
    s = sequences("strict")[0]
    cfg = dict(s["cfg"], scheme=hc.GODUNOV)
    rows, cols = cfg["rows"], cfg["cols"]
    cells = np.array([1 * cols + 1, 2 * cols + 2], np.uint64)
    twin = ha.StepTwin(cfg)
    twin.upload(cfg["st"], cfg["bed"], cfg["man"]); twin.set_target(1e9)
    twin.bed_shape_add(cells, cfg["bed"].reshape(-1)[cells.astype(int)].astype(np.float64) - 0.3, np.array([[0.0, 0.0], [1e-3, 1.0]]))
    twin.add_links([dict(a=1 * cols + 2, b=3 * cols + 3, kind=ha.PUMP, level=-50.0, size=0.01)])
    twin.step_batch(3)
    twin.save()
    state, bed, rec, sc, phase = twin.download(), twin.bed.copy(), twin.links_records(), twin.scalars(), twin.use_alt
    twin.bed_apply(); twin.step_batch(2)
    assert not np.array_equal(twin.bed, bed) and twin.use_alt == 0
    twin.restore()
    assert np.array_equal(twin.download(), state) and np.array_equal(twin.bed, bed) and twin.scalars() == sc and twin.use_alt == phase
    assert twin.links_records().tobytes() == rec.tobytes() and twin.warnings() == 0
    twin.bed_apply(); moved = twin.bed.copy()
    twin.bed_shapes_clear(); twin.clear_boundaries()
    twin.add_links([dict(a=1 * cols + 2, b=3 * cols + 3, kind=ha.PUMP, level=-50.0, size=0.01)])
    twin.step_batch(1)
    twin.restore()
    assert np.array_equal(twin.bed, moved) and twin.warnings() == 2 and not twin.links_records()["active"].any()
    assert np.array_equal(twin.download(), state)
