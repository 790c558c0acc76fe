"""Host-call sequences that move the bed and link cells, with iteration pairs forced on (tests/host_calls_actors.py draws them and
holds the stepwise twin, tests/host_calls_actors_worker.py runs them on the engine).

hp_bed_apply and link groups change the grid between the flux kernels, and both are wired into the engine's between-launch
bookkeeping (csrc/hp_facts.hpp): an apply is "bed uploaded, state uploaded"; a link group makes the domain unfusable, switches
pairs and speculation off and splits the merged bdy_area launch; hp_boundary_clear switches all of that back on; a checkpoint
carries the bed at the listed cells and the links' records, each with an "added or cleared since" rule.  Three legs of 60 seeds, in
chunks of 30 per worker process, mix these calls into the sequences of test_gpu_host_calls.py, and two hand-written scenarios name
the two meetings the fuzz is about:

* STRICT == the stepwise twin, bit for bit: state, bed and links' records at every download, the records at every links_read,
  time, timestep, hydrological time, counters, and the number of checkpoint warnings; pairs forced on;
* the same with every second speculative batch replayed (HP_STRICT_SPECULATE=1 HP_STRICT_SPEC_FORCE=2), fp64;
* FAST with exact pairs (HP_PAIR_EXACT=1) == FAST with pairs off, line for line (bed and records included), and the pairs run's
  final state within FAST's own bar of the twin wherever the twin can follow the sequence and, in fp32, agrees with its own fp64
  run to a tenth of the bar.  The links' records are held to the pairs-off run only: a branch of link_flow may flip on a last bit.

Every leg also asserts that the paths it is about really ran (applies that changed cells, links that moved water, pairs on the
seeds whose operations count a pairs pattern, no pair while a link group was attached, replays)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import host_calls as hc
import host_calls_actors as ha
from test_gpu_host_calls import FAST_RMSE_BAR, FAST_TIME_BAR, LEG_ENV, SKIP_CAP

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(__file__), "host_calls_actors_worker.py")
CHUNKS = list(range(0, ha.SEEDS_PER_LEG, ha.CHUNK))
COUNTERS = ("launches", "iterations", "pairs", "replays", "applies", "changed", "links_active", "pairs_with_links")


def worker(args, env, timeout=180):
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("HP_TWO_STEP", "HP_PAIR_", "HP_STRICT_SPEC", "HP_FILL_AFTER_PAIRS"))}
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=dict(clean, **env))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def fuzz_lines(leg, first, env, outdir=None):
    lines = [l for l in worker(["fuzz", leg, first, ha.CHUNK] + ([outdir] if outdir else []), env) if l.startswith("seed ")]
    assert len(lines) == ha.CHUNK
    return lines


def observed(line):
    return line.split("  # ")[0].split(" ", 2)[2]


def counters(line):
    words = line.split("  # ")[1].split()
    return {k: int(v) for k, v in zip(words[0::2], words[1::2])}


def total(lines):
    return {k: sum(counters(l)[k] for l in lines) for k in COUNTERS}


@functools.lru_cache(maxsize=None)
def sequences(leg, first):
    return [ha.make_actor_sequence(ha.SEED_BASE[leg] + i, leg) for i in range(first, first + ha.CHUNK)]


@functools.lru_cache(maxsize=None)
def twin_runs(leg, first):
    return [ha.run_on_twin(s) if s["twin_ok"] else None for s in sequences(leg, first)]


def the_paths_ran(lines, seqs):
    """From the worker's counters: applies that changed cells, links that moved water, pairs on a seed of each pairs pattern the
    chunk's operations count, and none while a link group was attached."""
    per_seed = [counters(l) for l in lines]
    assert any(c["applies"] > 0 and c["changed"] > 0 for c in per_seed), per_seed
    assert any(c["links_active"] > 0 for c in per_seed), per_seed
    assert all(c["pairs_with_links"] == 0 for c in per_seed), per_seed
    for pattern in ("pairs_after_links_cleared", "apply_between_pair_batches"):
        on = [c["pairs"] for c, s in zip(per_seed, seqs) if s["patterns"][pattern]]
        assert not on or max(on) > 0, (pattern, on)
    return per_seed


# ---- the fuzz legs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", CHUNKS)
@pytest.mark.parametrize("leg", ["strict", "spec"])
def test_strict_with_actors_equals_the_twin_bit_for_bit(leg, first):
    """Every comparison point (state, bed, records), the scalars and the number of checkpoint warnings equal the twin's; leg "spec"
    replays every second speculative batch -- none of them while a link group is attached, and an apply or a group added straight
    behind one resolves it first."""
    lines = fuzz_lines(leg, first, LEG_ENV[leg])
    seqs, refs = sequences(leg, first), twin_runs(leg, first)
    skipped = 0
    for line, seq, ref in zip(lines, seqs, refs):
        if not ref["finite"]:
            skipped += 1
            print(f"not compared, the twin's own run is not finite: seed {seq['cfg']['seed']} {ha.describe(seq)}")
            continue
        assert observed(line) == ha.digest(ref), f"seed {seq['cfg']['seed']}: {ha.describe(seq)}\nengine {observed(line)}\ntwin   {ha.digest(ref)}"
    assert skipped <= SKIP_CAP * ha.CHUNK
    c = total(lines)
    print(f"{leg} seeds {first}..{first + ha.CHUNK - 1}: held {ha.CHUNK - skipped}, left out {skipped}; {c}")
    the_paths_ran(lines, seqs)
    assert c["pairs"] > 0
    if leg == "spec":
        assert c["replays"] >= 1, c


@pytest.mark.parametrize("first", CHUNKS)
def test_fast_with_actors_and_exact_pairs_equals_fast_without_pairs(first, tmp_path):
    """Every observable of the run with pairs forced on (exact flavour) equals the run with pairs off: state, bed and links'
    records at every comparison point, the scalars, the warnings.  The final state of the pairs run is also held to the stepwise
    twin at FAST's own bar on the seeds the twin can follow (no partial upload, no set_time); an fp32 run where the fp32 twin stays
    within a tenth of the bar of its own fp64 run (host_calls_actors.reference_error).
    Largest depth RMSE against the twin measured on an MI355X over the 60 seeds: 5.6e-15 m in fp64 (20 seeds held), 6.4e-7 m in
    fp32 (7 held, 4 left out for the twin's own fp32 rounding of 1.6e-5 ... 8.1e-4 m); no run was left out as not finite."""
    off = fuzz_lines("fast", first, dict(HP_TWO_STEP="0", HP_PAIR_EXACT="1"))
    on = fuzz_lines("fast", first, LEG_ENV["fast"], str(tmp_path))
    seqs = sequences("fast", first)
    blown = 0
    for a, b, seq in zip(off, on, seqs):
        assert observed(a) == observed(b), f"seed {seq['cfg']['seed']}: {ha.describe(seq)}\npairs off {observed(a)}\npairs on  {observed(b)}"
        if "non-finite" in observed(b):
            blown += 1
            print(f"not compared, the run is not finite: seed {seq['cfg']['seed']} {ha.describe(seq)}")
    assert blown <= SKIP_CAP * ha.CHUNK
    worst, held = {"f64": 0.0, "f32": 0.0}, {"f64": 0, "f32": 0}
    for i, (line, seq, ref) in enumerate(zip(on, seqs, twin_runs("fast", first))):
        if ref is None or not ref["finite"] or "non-finite" in observed(line):
            continue
        prec = seq["cfg"]["precision"]
        ref_err = ha.reference_error(seq, ref)
        if ref_err >= hc.REFERENCE_ERROR_SHARE * FAST_RMSE_BAR[prec]:
            print(f"not held to the twin, whose own fp32 rounding moves it by {ref_err:.3e} m (host_calls_actors.reference_error): seed {seq['cfg']['seed']} {ha.describe(seq)}")
            continue
        got = np.load(os.path.join(str(tmp_path), f"fast_{first + i}.npy"))
        rmse = hc.depth_rmse(got, ref["points"][-1][0], ref["bed"])
        t_eng, t_ref = float(observed(line).split(" | ")[2].split()[0]), float(ref["scalars"][0])
        worst[prec] = max(worst[prec], rmse)
        held[prec] += 1
        what = f"seed {seq['cfg']['seed']}: {ha.describe(seq)}"
        assert rmse < FAST_RMSE_BAR[prec], (rmse, what)
        assert abs(t_eng - t_ref) <= FAST_TIME_BAR[prec] * abs(t_ref), (t_eng, t_ref, what)
    c_on, c_off = total(on), total(off)
    print(f"fast seeds {first}..{first + ha.CHUNK - 1}: pairs on {c_on}; pairs off {c_off}; left out as not finite {blown}; held to the twin "
          f"{held['f64']} fp64 and {held['f32']} fp32 seeds, largest depth RMSE fp64 {worst['f64']:.3e} m fp32 {worst['f32']:.3e} m")
    assert c_off["pairs"] == 0 and c_on["pairs"] > 0 and c_on["launches"] < c_off["launches"], (c_on, c_off)
    the_paths_ran(on, seqs)
    assert held["f64"] + held["f32"] >= 5


# ---- two meetings, by hand ------------------------------------------------------------------------------------------------------------
def scenario(name, tmp_path, env):
    out = os.path.join(str(tmp_path), f"{name}_{env.get('HP_TWO_STEP', 'x')}.npz")
    worker(["scenario", name, out], env)
    return np.load(out)


def twin_scenario(name):
    twin = ha.StepTwin(ha.scenario_cfg(name))
    return ha.run_scenario(name, twin), twin


def test_pairs_resume_when_the_last_link_group_is_cleared(tmp_path):
    """FAST fp64 64 x 37 rough terrain under rain: batch(8), a link group, batch(7), hp_boundary_clear, batch(8).  The group takes
    the domain off pairs (the other buffer is repaired, the rain leaves the flux kernel for a pass of its own) and the clear puts it
    back on them: pairs in the first and the last batch and none in the middle, every bit -- state, bed, records, scalars -- that of
    the run with pairs off, and the final state within FAST's bar of the twin."""
    name = "pairs_resume_after_links_cleared"
    off = scenario(name, tmp_path, dict(HP_TWO_STEP="0", HP_PAIR_EXACT="1"))
    on = scenario(name, tmp_path, dict(HP_TWO_STEP="1", HP_PAIR_EXACT="1"))
    assert on["pairs"][0] >= 2 and on["pairs"][1] == 0 and on["pairs"][2] >= 2 and list(off["pairs"]) == [0, 0, 0], (on["pairs"], off["pairs"])
    for key in ("states", "beds", "scalars", "records"):
        assert np.array_equal(on[key], off[key]), key
    ref, twin = twin_scenario(name)
    moved = int(ref["records"][0]["active"].sum())
    assert moved > 0 and int(on["records"].view(ha_record_dtype())["active"].sum()) > 0
    rmse = hc.depth_rmse(on["states"][-1], ref["states"][-1], ref["beds"][-1])
    t_ref = ref["scalars"][-1][0]
    print(f"{name}: pairs per batch {list(on['pairs'])}, links active {moved}, depth RMSE vs the twin {rmse:.3e} m, time {on['scalars'][-1][0]!r} vs {t_ref!r}")
    assert rmse < FAST_RMSE_BAR["f64"] and abs(on["scalars"][-1][0] - t_ref) <= FAST_TIME_BAR["f64"] * t_ref


def ha_record_dtype():
    import hipims_mi as hp
    return hp.LINK_RECORD_DTYPE


def test_an_apply_behind_replayed_batches_and_a_restore_across_it_are_the_twin(tmp_path):
    """STRICT fp64 65 x 37 terrain with dry ground and null cells, every speculative batch replayed: batch(9), hp_bed_apply with a
    breach that is opening and a barrier that is rising at that time, batch(5), save, batch(9), hp_bed_apply, restore, batch(9).
    The apply has to patch the state the replay left, not the speculative one; the short batch runs pairs on the buffers the
    apply wrote; the restore brings back the bed of the listed cells with the levels that stand on it.  State, bed and scalars
    after every batch and after the second apply equal the twin's in every bit."""
    name = "apply_behind_replayed_batches"
    got = scenario(name, tmp_path, dict(HP_TWO_STEP="1", HP_STRICT_SPECULATE="1", HP_STRICT_SPEC_FORCE="1"))
    ref, twin = twin_scenario(name)
    assert twin.applies == 2 and twin.changed_total > 20 and not np.array_equal(ref["beds"][0], ref["beds"][1])
    assert not np.array_equal(ref["beds"][2], ref["beds"][3]) and np.array_equal(ref["beds"][4], ref["beds"][2])      # the second apply moved it, the restore took that back
    for i in range(len(ref["states"])):
        assert np.array_equal(got["states"][i], ref["states"][i]), f"state at point {i}"
        assert np.array_equal(got["beds"][i], ref["beds"][i]), f"bed at point {i}"
        assert list(got["scalars"][i]) == list(ref["scalars"][i]), (i, got["scalars"][i], ref["scalars"][i])
    print(f"{name}: pairs per batch {list(got['pairs'])}, replays {int(got['replays'])}, applies {int(got['applies'])}, cells changed {int(got['changed_total'])}")
    assert int(got["applies"]) == 2 and int(got["changed_total"]) == twin.changed_total and int(got["warnings"]) == ref["warnings"] == 0
    assert got["pairs"][1] >= 1, got["pairs"]                                    # (the short batch behind the apply ran pairs)
    assert int(got["replays"]) == 3                                             # (three batches of 9: all speculative, all replayed)
