"""Worker of tests/test_gpu_plan_counts.py: a fingerprint of the engine's launch decisions (hp_plan.hpp) through the Python API alone, so
that the same file runs unchanged on the commit before the decisions moved.  The switches are read once per process: every scenario
is a process of its own, with no HP_* variable but its own and HP_PAIR_TUNE=0 (the tuner's choice depends on timing).
usage: plan_counts_worker.py <scenario>             one scenario: prints its result as one JSON line
       plan_counts_worker.py --record <commit>      every scenario, each in a child with a time limit: prints what
                                                    tests/plan_counts_expected.json holds, <commit> being the commit the library was built from
After every call of a scenario's plan the line holds launch_counts(), pair_stats()'s pairs and cold starts and the iteration count; at
its end a SHA-256 over the downloaded state and the scalars."""
import hashlib
import json
import os
import subprocess
import sys

BATCHES = (1, 2, 7, 8)
RUNS = [("run", n) for n in BATCHES]
# name -> (environment, domain, plan); grids are 96 x 64 unless the domain says otherwise
SCENARIOS = {
    "f64_fast":          ({"HP_TWO_STEP": "1"}, {}, RUNS),
    "f64_rain":          ({"HP_TWO_STEP": "1"}, {}, [("rain",)] + RUNS),        # fused: cold start, then warm pairs, a batch's last pair not followed
    "f64_loss":          ({"HP_TWO_STEP": "1"}, {}, [("loss",)] + RUNS),        # a boundary that removes water: exact pairs by default
    "f64_strict":        ({"HP_TWO_STEP": "1"}, {"math": "strict"}, RUNS),
    "f32_rain":          ({}, {"precision": "f32"}, [("rain",)] + RUNS),
    "f32_rain_two_step": ({"HP_TWO_STEP": "1"}, {"precision": "f32"}, [("rain",)] + RUNS),
    "muscl_5x5":         ({"HP_TWO_STEP": "1"}, {"scheme": "muscl", "cols": 5, "rows": 5}, RUNS),
    "muscl":             ({"HP_TWO_STEP": "1"}, {"scheme": "muscl"}, RUNS),
    "inertial_3x3":      ({"HP_TWO_STEP": "1"}, {"scheme": "inertial", "cols": 3, "rows": 3}, RUNS),
    "inertial":          ({"HP_TWO_STEP": "1"}, {"scheme": "inertial"}, RUNS),
    "basic":             ({"HP_TWO_STEP": "1"}, {"kernel": "basic"}, RUNS),
    "fixed_dt":          ({"HP_TWO_STEP": "1"}, {"fixed": True}, RUNS),
    "q1_off":            ({"HP_TWO_STEP": "1"}, {"q1": False}, RUNS),
    "launch_tail_0":     ({"HP_TWO_STEP": "1", "HP_LAUNCH_TAIL": "0"}, {}, RUNS),
    "fill_after_pairs_0": ({"HP_TWO_STEP": "1", "HP_FILL_AFTER_PAIRS": "0"}, {}, RUNS),
    "upload_rows":       ({"HP_TWO_STEP": "1"}, {"by_rows": 16}, RUNS),         # a whole grid in blocks of 16 rows: the ring comparison lets it pair
    "split_steps":       ({"HP_TWO_STEP": "1"}, {}, [("rain",), ("run", 8), ("split",), ("split",), ("run", 8)]),
    "save_restore":      ({"HP_TWO_STEP": "1"}, {}, [("run", 8), ("save",), ("run", 3), ("restore",), ("run", 8)]),
}


def run_scenario(name):
    import numpy as np

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "hipims-ocl_amd")]
    import hipims_mi as hp
    from hipims_mi import synthetic as syn

    _, dom_kw, plan = SCENARIOS[name]
    cols, rows = dom_kw.get("cols", 96), dom_kw.get("rows", 64)
    precision = dom_kw.get("precision", "f64")
    real = np.float64 if precision == "f64" else np.float32
    scheme = {"godunov": hp.SCHEME_GODUNOV, "muscl": hp.SCHEME_MUSCL_HANCOCK, "inertial": hp.SCHEME_INERTIAL}[dom_kw.get("scheme", "godunov")]
    if min(cols, rows) < 8 or scheme == hp.SCHEME_INERTIAL:                  # (the inertial scheme is only meaningful for a gentle step)
        st, bed, man = syn.s_dam(cols, rows, dtype=real, levels=(1.2, 1.0))
    else:
        st, bed, man = syn.s_rough(cols, rows, dtype=real, manning=None)
    kw = dict(dynamic_dt=False, dt_fixed=0.01) if dom_kw.get("fixed") else {}
    dom = hp.Domain(cols, rows, scheme=scheme, precision=precision,
                    math_mode=hp.MATH_STRICT if dom_kw.get("math") == "strict" else hp.MATH_FAST,
                    kernel=hp.KERNEL_BASIC if dom_kw.get("kernel") == "basic" else hp.KERNEL_AUTO,
                    quirks=hp.QUIRKS_REFERENCE if dom_kw.get("q1", True) else hp.QUIRKS_REFERENCE & ~hp.QUIRK_CFL_READS_PRIMARY, **kw)
    if "by_rows" in dom_kw:
        dom.upload(bed=bed, manning=man)
        for row0 in range(0, rows, dom_kw["by_rows"]):
            dom.upload_rows(st[row0:row0 + dom_kw["by_rows"]], row0)
    else:
        dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    trail = []
    for step in plan:
        if step[0] == "run":
            dom.step_batch(step[1])
        elif step[0] == "rain":
            dom.add_uniform(hp.UNIFORM_RAIN_INTENSITY, np.array([[0.0, 600.0], [30.0, 200.0], [60.0, 0.0], [90.0, 0.0]]), 30.0, 90.0)
            assert dom.boundaries_fused()
        elif step[0] == "loss":
            dom.add_uniform(hp.UNIFORM_LOSS_RATE, np.array([[0.0, 900.0], [1000.0, 900.0]]), 1000.0, 1000.0)
            assert dom.boundaries_fused()
        elif step[0] == "split":
            dom.step_begin()
            dom.step_end()
        elif step[0] == "save":
            dom.state_save()
        elif step[0] == "restore":
            dom.state_restore()
        sc = dom.read_scalars()
        ps = dom.pair_stats()
        trail.append([step[0], list(dom.launch_counts()), [ps["pairs"], ps["cold_starts"]], sc["iterations"]])
    state = dom.download()
    sc = dom.read_scalars()
    digest = hashlib.sha256(state.tobytes())
    digest.update(json.dumps({k: (float(v).hex() if isinstance(v, float) else int(v)) for k, v in sorted(sc.items())}).encode())
    dom.close()
    return {"trail": trail, "sha256": digest.hexdigest()}


def compact(recording):
    """The recording as JSON with one call of a scenario's plan per line: a count that moves shows as one changed line."""
    lines = ['{"commit": %s, "scenarios": {' % json.dumps(recording["commit"])]
    names = list(recording["scenarios"])
    for name in names:
        r = recording["scenarios"][name]
        lines.append(' %s: {"trail": [' % json.dumps(name))
        lines += ["  " + json.dumps(step) + ("," if i + 1 < len(r["trail"]) else "") for i, step in enumerate(r["trail"])]
        lines.append('  ], "sha256": %s}%s' % (json.dumps(r["sha256"]), "," if name != names[-1] else ""))
    return "\n".join(lines + ["}}"])


def child_environment(name):
    """The caller's environment without any of the library's switches, plus the scenario's own."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("HP_")}
    return dict(env, HP_PAIR_TUNE="0", **SCENARIOS[name][0])


def run_child(name, timeout=120):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, timeout=timeout, env=child_environment(name))
    assert r.returncode == 0, (name, r.stdout[-2000:] + r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    if sys.argv[1] == "--record":
        recorded = {}
        for name in SCENARIOS:                              # (a child that fails ends the recording: nothing more is started)
            recorded[name] = run_child(name)
            print(name, recorded[name]["trail"][-1], file=sys.stderr, flush=True)
        print(compact({"commit": sys.argv[2], "scenarios": recorded}))
    else:
        print(json.dumps(run_scenario(sys.argv[1])))
