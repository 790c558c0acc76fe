"""Mixed host-call sequences with iteration pairs forced on (tests/host_calls.py draws them, tests/host_calls_worker.py runs them).

The engine's state between launches is ten host-side facts that the entry points change by naming what happened to the device
(csrc/hp_facts.hpp, pinned event by event in test_facts.py); every finding of the round-6 review was a call sequence that
left one of them wrong, when each entry point still set and cleared them by hand.  Three fuzz legs of 120 seeds each, in chunks of 30 per
worker process, mix everything the host can call with HP_TWO_STEP=1, and four hand-written regressions name the findings:

* STRICT == the oracle, bit for bit (state at every download, time, timestep, hydrological time, counters), pairs forced on;
* the same with every second speculative batch replayed (HP_STRICT_SPECULATE=1 HP_STRICT_SPEC_FORCE=2), fp64;
* FAST with exact pairs (HP_PAIR_EXACT=1) == FAST with pairs off, line for line, and the pairs run's final state within FAST's own
  bar of the oracle wherever the oracle can follow the sequence and, in fp32, agrees with its own fp64 run to a tenth of the bar
  (depth RMSE < 1e-9 m fp64 / 1e-4 m fp32, time within 1e-12 / 1e-5).

Every leg also asserts that the paths it is about really ran (pairs, cold starts, stamps, replays)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import hipims_mi as hp
import oracle
from hipims_mi import synthetic as syn

import host_calls as hc

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(__file__), "host_calls_worker.py")
CHUNKS = list(range(0, hc.SEEDS_PER_LEG, hc.CHUNK))
PAIRS_ON = dict(HP_TWO_STEP="1")
LEG_ENV = {"strict": PAIRS_ON, "spec": dict(PAIRS_ON, HP_STRICT_SPECULATE="1", HP_STRICT_SPEC_FORCE="2"), "fast": dict(PAIRS_ON, HP_PAIR_EXACT="1")}
SKIP_CAP = 0.05                                            # share of a leg's seeds that may go uncompared (non-finite runs): test_host_calls_cpu.py


def worker(args, env, timeout=180):
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("HP_TWO_STEP", "HP_PAIR_", "HP_STRICT_SPEC", "HP_FILL_AFTER_PAIRS"))}
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=dict(clean, **env))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def fuzz_lines(leg, first, env, outdir=None):
    lines = [l for l in worker(["fuzz", leg, first, hc.CHUNK] + ([outdir] if outdir else []), env) if l.startswith("seed ")]
    assert len(lines) == hc.CHUNK
    return lines


def observed(line):
    return line.split("  # ")[0].split(" ", 2)[2]


def counters(lines):
    total = dict.fromkeys(("launches", "iterations", "pairs", "cold_starts", "stamped", "replays"), 0)
    for l in lines:
        words = l.split("  # ")[1].split()
        for k, v in zip(words[0::2], words[1::2]):
            total[k] += int(v)
    return total


@functools.lru_cache(maxsize=None)
def sequences(leg, first):
    return [hc.make_sequence(hc.SEED_BASE[leg] + i, leg) for i in range(first, first + hc.CHUNK)]


@functools.lru_cache(maxsize=None)
def oracle_runs(leg, first):
    return [hc.run_on_oracle(s) if s["oracle_ok"] else None for s in sequences(leg, first)]


@functools.lru_cache(maxsize=None)
def reference_errors(leg, first):
    return [hc.reference_error(s, r) if r is not None and r["finite"] else None for s, r in zip(sequences(leg, first), oracle_runs(leg, first))]


def patterns(leg):
    total = dict.fromkeys(hc.PATTERNS, 0)
    for first in CHUNKS:
        for s in sequences(leg, first):
            for k, v in s["patterns"].items():
                total[k] += v
    return total


# ---- the fuzz legs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", CHUNKS)
@pytest.mark.parametrize("leg", ["strict", "spec"])
def test_strict_with_pairs_equals_the_oracle_bit_for_bit(leg, first):
    """STRICT pairs run where there are no boundaries, single iterations behind them; leg "spec" replays every second speculative batch.
    At least 8 % of a chunk's iterations must have run as pairs: about 70 % of the seeds are Godunov, half of those without boundaries,
    85 % of those with a dynamic timestep -- 30 % of the seeds can pair -- and split steps, odd batches and the single iterations behind
    uploads leave about half of their iterations to pairs, 15 %; half of that is the floor.  Leg "spec": a speculative batch (8 iterations
    and more) runs no pairs, which leaves the batches of 1, 2, 3 and 7 -- 13 of the 95 iterations of one draw of each size -- so a
    seventh of the above: 2 %, and 1 % is the floor."""
    lines = fuzz_lines(leg, first, LEG_ENV[leg])
    seqs, refs = sequences(leg, first), oracle_runs(leg, first)
    skipped = 0
    for line, seq, ref in zip(lines, seqs, refs):
        if not ref["finite"]:
            skipped += 1
            print(f"not compared, the oracle's own run is not finite: seed {seq['cfg']['seed']} {hc.describe(seq)}")
            continue
        assert observed(line) == hc.digest(ref), f"seed {seq['cfg']['seed']}: {hc.describe(seq)}\nengine {observed(line)}\noracle {hc.digest(ref)}"
    assert skipped <= SKIP_CAP * hc.CHUNK
    c = counters(lines)
    print(f"{leg} seeds {first}..{first + hc.CHUNK - 1}: {c}, launches / iterations {c['launches'] / c['iterations']:.3f}, patterns in the leg {patterns(leg)}")
    assert 2 * c["pairs"] >= (0.08 if leg == "strict" else 0.01) * c["iterations"], c
    assert c["cold_starts"] == 0                                   # (STRICT pairs carry no boundaries: nothing to start cold)
    if leg == "spec":
        assert c["replays"] >= 1, c
        assert patterns(leg)["speculation_after_short_pairs"] >= 1
    assert patterns(leg)["boundary_change_in_checkpoint"] >= 1


FAST_RMSE_BAR, FAST_TIME_BAR = {"f64": 1e-9, "f32": 1e-4}, {"f64": 1e-12, "f32": 1e-5}


@pytest.mark.parametrize("first", CHUNKS)
def test_fast_with_exact_pairs_equals_fast_without_pairs(first, tmp_path):
    """The project's bar for pairs: every observable of the run with pairs forced on (exact flavour) equals the run with pairs off.  The
    final state of the pairs run is also held to the oracle at FAST's own bar on the seeds the oracle can follow.  At least 20 % of a
    chunk's iterations must have run as pairs (70 % of the seeds are Godunov, nearly all of them with a dynamic timestep; cell boundaries,
    split steps, odd batches and the single iterations behind uploads take more than half of that away), and the boundary seeds must have
    started cold and written stamps.
    An fp32 run is held to the fp32 oracle where the oracle itself stays within a tenth of the bar of its own fp64 run
    (host_calls.reference_error: on a few sequences fp32 rounding alone moves the oracle by 2e-4 ... 5e-1 m, and it measures nothing at
    1e-4 m); the seeds left out are printed with that figure and still held to the run with pairs off.
    Largest depth RMSE against the oracle measured on an MI355X over the 120 seeds: 8.8e-16 m in fp64 (34 seeds held), 4.6e-6 m in fp32
    (10 held, 4 left out: seed 15040 is 1.57e-4 m from the fp32 oracle, which is itself 2.16e-4 m from its fp64 run -- the two part at
    the same cell, (16, 57), by the same 9.70e-4 m after 20 iterations, where the FAST run has the fp64 oracle's depth to six digits)."""
    off = fuzz_lines("fast", first, dict(HP_TWO_STEP="0", HP_PAIR_EXACT="1"))
    on = fuzz_lines("fast", first, LEG_ENV["fast"], str(tmp_path))
    seqs = sequences("fast", first)
    blown = 0
    for a, b, seq in zip(off, on, seqs):
        assert observed(a) == observed(b), f"seed {seq['cfg']['seed']}: {hc.describe(seq)}\npairs off {observed(a)}\npairs on  {observed(b)}"
        if "non-finite" in observed(b):
            blown += 1
            print(f"not compared, the run is not finite: seed {seq['cfg']['seed']} {hc.describe(seq)}")
    assert blown <= SKIP_CAP * hc.CHUNK
    worst = {"f64": 0.0, "f32": 0.0}
    held = 0
    for i, (line, seq, ref, ref_err) in enumerate(zip(on, seqs, oracle_runs("fast", first), reference_errors("fast", first))):
        if ref is None or not ref["finite"] or "non-finite" in observed(line):
            continue
        prec = seq["cfg"]["precision"]
        if ref_err >= hc.REFERENCE_ERROR_SHARE * FAST_RMSE_BAR[prec]:
            print(f"not held to the oracle, whose own fp32 rounding moves it by {ref_err:.3e} m (host_calls.reference_error): seed {seq['cfg']['seed']} {hc.describe(seq)}")
            continue
        got = np.load(os.path.join(str(tmp_path), f"fast_{first + i}.npy"))
        rmse = hc.depth_rmse(got, ref["points"][-1], ref["bed"])
        t_eng, t_ref = float(observed(line).split(" | ")[1].split()[0]), float(ref["scalars"][0])
        worst[prec] = max(worst[prec], rmse)
        held += 1
        what = f"seed {seq['cfg']['seed']}: {hc.describe(seq)}"
        assert rmse < FAST_RMSE_BAR[prec], (rmse, what)
        assert abs(t_eng - t_ref) <= FAST_TIME_BAR[prec] * abs(t_ref), (t_eng, t_ref, what)
    c_on, c_off = counters(on), counters(off)
    print(f"fast seeds {first}..{first + hc.CHUNK - 1}: pairs on {c_on}, launches / iterations {c_on['launches'] / c_on['iterations']:.3f} (pairs off "
          f"{c_off['launches'] / c_off['iterations']:.3f}); held to the oracle {held} seeds, largest depth RMSE fp64 {worst['f64']:.3e} m fp32 {worst['f32']:.3e} m; "
          f"patterns in the leg {patterns('fast')}")
    assert c_off["pairs"] == 0
    assert 2 * c_on["pairs"] >= 0.2 * c_on["iterations"] and c_on["launches"] < 0.9 * c_off["launches"], (c_on, c_off)
    assert c_on["cold_starts"] >= 1 and c_on["stamped"] >= 1, c_on
    assert held >= 5
    p = patterns("fast")
    assert p["split_after_boundary_pairs"] >= 1 and p["boundary_change_in_checkpoint"] >= 1 and p["blocks_then_batch"] >= 1, p


# ---- the four findings, by hand -------------------------------------------------------------------------------------------------------
def scenario(name, tmp_path, env):
    out = os.path.join(str(tmp_path), f"{name}_{env.get('HP_TWO_STEP', 'x')}.npz")
    worker(["scenario", name, out], env)
    return np.load(out)


def rain_oracle(second_rain_at_8):
    st, bed, man = syn.s_rough(64, 37, manning=None, seed=31)
    ref = oracle.OracleSim(64, 37)
    ref.upload(st, bed, man)
    ref.add_uniform(hp.UNIFORM_RAIN_INTENSITY, np.array([[0.0, 600.0], [0.7, 200.0], [1.4, 50.0], [2.1, 0.0]]), 0.7, 2.1)
    ref.set_target(1e9)
    ref.run(8)
    if second_rain_at_8:                                       # (the boundary list is not part of a checkpoint: the rain added inside it stays)
        ref.add_uniform(hp.UNIFORM_RAIN_INTENSITY, np.array([[0.0, 5000.0], [0.7, 3000.0], [1.4, 0.0], [2.1, 0.0]]), 0.7, 2.1)
    else:
        ref.run(2)
    ref.run(8)
    return ref, bed


@pytest.mark.parametrize("name", ["split_behind_boundary_pairs", "boundary_change_in_checkpoint"])
def test_pairs_with_rain_survive_split_steps_and_a_boundary_change_in_a_checkpoint(name, tmp_path):
    """FAST fp64 64 x 37 wet/dry terrain under uniform rain.  (1) batch(8), two split steps, batch(8): hp_step_begin has to forget the
    maximum the last boundary pair priced (SLOT_M1), or the next batch's first pair advances with a timestep two iterations old.
    (2) batch(8), save, a second and stronger rain, restore, batch(8): the restore must not bring back a maximum priced under the old
    boundary set.  Equal to the run with pairs off in state, time and timestep; within FAST's bar of the oracle; pairs in both batches."""
    off = scenario(name, tmp_path, dict(HP_TWO_STEP="0", HP_PAIR_EXACT="1"))
    on = scenario(name, tmp_path, dict(HP_TWO_STEP="1", HP_PAIR_EXACT="1"))
    # (pairs in both batches -- the first iterations behind an upload are single ones; a cold start in front of each batch's first pair)
    assert min(on["pairs"]) >= 2 and list(off["pairs"]) == [0, 0], (on["pairs"], off["pairs"])
    assert int(on["cold_starts"]) >= 2, int(on["cold_starts"])
    assert np.array_equal(on["scalars"], off["scalars"]), (on["scalars"], off["scalars"])
    assert np.array_equal(on["states"], off["states"])
    ref, bed = rain_oracle(name == "boundary_change_in_checkpoint")
    rmse = hc.depth_rmse(on["states"][-1], ref.download(), bed)
    t_ref = ref.scalars()["t"]
    print(f"{name}: depth RMSE vs the oracle {rmse:.3e} m, time {on['scalars'][-1][0]!r} vs {t_ref!r}")
    assert rmse < 1e-9 and abs(on["scalars"][-1][0] - t_ref) <= 1e-12 * t_ref


def test_a_replay_behind_pairs_is_still_the_oracle(tmp_path):
    """STRICT fp64 65 x 37 terrain with dry ground and null cells, every speculative batch replayed: 6, 9, 5, 12 iterations.  The short
    batches run pairs and leave the other buffer two iterations old; the snapshot in front of a speculative batch has to be taken with
    that buffer repaired, or the replay restores a stale buffer marked as current and the cells the reference leaves untouched (Q3)
    continue from the wrong value."""
    got = scenario("replay_behind_pairs", tmp_path, dict(HP_TWO_STEP="1", HP_STRICT_SPECULATE="1", HP_STRICT_SPEC_FORCE="1"))
    st, bed, man = hc.rough_with_nulls(65, 37)
    assert ((st[..., 0] - bed <= 1e-3) & (st[..., 1] > -9000))[1:-1, 1:-1].sum() > 100          # dry ground is really there
    ref = oracle.OracleSim(65, 37)
    ref.upload(st, bed, man)
    ref.set_target(1e9)
    for i, n in enumerate((6, 9, 5, 12)):
        ref.run(n)
        sr = ref.scalars()
        assert np.array_equal(got["states"][i], ref.download()), f"after batch {i} ({n} iterations)"
        assert got["scalars"][i][0] == sr["t"] and got["scalars"][i][1] == sr["dt"], (i, got["scalars"][i], sr)
    print(f"replay behind pairs: pairs per batch {list(got['pairs'])}, replays {int(got['replays'])}, stamped cells {int(got['stamped_ever'])}")
    assert got["pairs"][0] >= 1 and got["pairs"][2] >= 1, got["pairs"]           # (the short batches ran pairs)
    assert int(got["replays"]) == 2                                             # (9 and 12 iterations: both speculative, both replayed)


def test_a_grid_loaded_block_by_block_still_pairs(tmp_path):
    """FAST fp64 130 x 64 dam break inside the usual closed wall ring, its state loaded through hp_domain_upload_rows alone, in blocks of
    16 rows: the two buffers' edge rings are compared once (rings_really_differ), found equal, and the batch runs in pairs -- the same
    bits as with pairs off.  Companion: rows written back after a run with water standing on the ring -- the rings differ, and
    whichever way the engine decides, the bits are those of the run with pairs off."""
    off = scenario("blockwise_load", tmp_path, dict(HP_TWO_STEP="0", HP_PAIR_EXACT="1"))
    on = scenario("blockwise_load", tmp_path, dict(HP_TWO_STEP="1", HP_PAIR_EXACT="1"))
    assert np.array_equal(on["states"], off["states"]) and np.array_equal(on["scalars"], off["scalars"])
    assert int(on["iterations"]) == 20 and int(on["launches"]) < 0.62 * int(on["iterations"]), (on["launches"], on["iterations"])
    off = scenario("blockwise_load_open_edge", tmp_path, dict(HP_TWO_STEP="0", HP_PAIR_EXACT="1"))
    on = scenario("blockwise_load_open_edge", tmp_path, dict(HP_TWO_STEP="1", HP_PAIR_EXACT="1"))
    assert np.array_equal(on["states"], off["states"]) and np.array_equal(on["scalars"], off["scalars"])
    assert on["pairs"][0] >= 1                                                  # (the run before the rows came back did pair)
    print(f"block-wise load, open edge: pairs per batch {list(on['pairs'])}")
