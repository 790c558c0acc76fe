"""Worker of tests/test_gpu_gridded_lookup.py (HP_TWO_STEP, HP_FUSE_BDY and HP_PAIR_EXACT are read once per process; the caller sets
them): runs every table row of tests/gridded_cases.py that applies to one PATH of the gridded lookup, rain intensity and mass flux, on
the STRICT and the FAST engine, next to oracle.OracleSim, and writes what it found as JSON -- per case and batch whether STRICT equals
the oracle in every bit of the state and of the time scalars (and the first cell that differs), FAST's depth error and time error
against the oracle, a digest of FAST's state and time scalars (the caller holds the paths to each other with it), and whether the
boundaries rode in the flux kernel and iteration pairs ran.
usage: gridded_lookup_worker.py <path> <precision> <out.json> [row-label-prefix]"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd"), os.path.dirname(os.path.abspath(__file__))]
import gridded_cases as gc  # noqa: E402
import hipims_mi as hp  # noqa: E402
import oracle  # noqa: E402

# path -> (resolutions, scheme, kernel, a loss rate in front, boundaries fused, pairs run)
PATHS = {
    "standalone": (gc.RES_FINE, hp.SCHEME_GODUNOV, hp.KERNEL_AUTO, False, False, None),
    "unfused": (gc.RES_FUSED, hp.SCHEME_GODUNOV, hp.KERNEL_AUTO, False, False, False),       # HP_FUSE_BDY=0 HP_TWO_STEP=0
    "unfused_loss": (gc.RES_FUSED, hp.SCHEME_GODUNOV, hp.KERNEL_AUTO, True, False, False),   # HP_FUSE_BDY=0 HP_TWO_STEP=0
    "inertial": (gc.RES_FUSED, hp.SCHEME_INERTIAL, hp.KERNEL_AUTO, False, False, None),
    "basic": (gc.RES_FUSED, hp.SCHEME_GODUNOV, hp.KERNEL_BASIC, False, False, None),
    "k1": (gc.RES_FUSED, hp.SCHEME_GODUNOV, hp.KERNEL_AUTO, False, True, False),             # HP_TWO_STEP=0
    "k1_loss": (gc.RES_FUSED, hp.SCHEME_GODUNOV, hp.KERNEL_AUTO, True, True, False),         # HP_TWO_STEP=0
    "k1b": (gc.RES_FUSED, hp.SCHEME_GODUNOV, hp.KERNEL_AUTO, False, True, True),             # HP_TWO_STEP=1
    "k1b_exact": (gc.RES_FUSED, hp.SCHEME_GODUNOV, hp.KERNEL_AUTO, False, True, True),       # HP_TWO_STEP=1 HP_PAIR_EXACT=1
    "k1b_loss": (gc.RES_FUSED, hp.SCHEME_GODUNOV, hp.KERNEL_AUTO, True, True, True),         # HP_TWO_STEP=1
}
LOSS = (np.array([[0.0, 90.0], [1000.0, 90.0]]), 1000.0, 1000.0)                             # mm/h, below most of the rain: land wets and dries
DX = 40.0


def attach(sim, loss, definition, grids, res, ox, oy):
    if loss:
        sim.add_uniform(hp.UNIFORM_LOSS_RATE, *LOSS)
    sim.add_gridded(definition, grids, res, ox, oy, gc.INTERVAL)


def run_oracle(precision, scheme, scene, *bdy):
    sim = oracle.OracleSim(gc.COLS, gc.ROWS, dx=DX, scheme=scheme, precision=precision, dt_initial=gc.DT0, threads=8)
    sim.upload(*scene)
    attach(sim, *bdy)
    sim.set_time(gc.T0)
    sim.set_target(1e9)
    out = []
    for step in gc.PLAN:
        if step == "download":
            sim.download()
            continue
        sim.run(step)
        sc = sim.scalars()
        out.append((sim.download(), sc["t"], sc["dt"]))
    return out


def run_engine(precision, scheme, kernel, math_mode, scene, *bdy):
    dom = hp.Domain(gc.COLS, gc.ROWS, dx=DX, scheme=scheme, precision=precision, math_mode=math_mode, kernel=kernel, dt_initial=gc.DT0)
    dom.upload(*scene)
    attach(dom, *bdy)
    fused = dom.boundaries_fused()
    dom.set_time(gc.T0)
    dom.set_target_time(1e9)
    out = []
    for step in gc.PLAN:
        if step == "download":
            dom.download()
            continue
        dom.step_batch(step)
        sc = dom.read_scalars()
        out.append((dom.download(), sc["time"], sc["timestep"]))
    pairs = (dom.pair_stats() or dict(pairs=0))["pairs"]
    dom.close()
    return out, fused, int(pairs)


def main(path, precision, out_file, only=""):
    resolutions, scheme, kernel, loss, _, _ = PATHS[path]
    real = np.float64 if precision == "f64" else np.float32
    scene = gc.scene(real)
    bed = scene[1].astype(np.float64)
    results = []
    for label, res, ox, oy, gr, gcols in gc.table(DX, real, resolutions):
        if not label.startswith(only):
            continue
        for definition in gc.DEFINITIONS:
            bdy = (loss, definition, gc.rates(definition, gc.SLICES, gr, gcols, real), res, ox, oy)
            ref = run_oracle(precision, scheme, scene, *bdy)
            strict, s_fused, s_pairs = run_engine(precision, scheme, kernel, hp.MATH_STRICT, scene, *bdy)
            fast, f_fused, f_pairs = run_engine(precision, scheme, kernel, hp.MATH_FAST, scene, *bdy)
            r = dict(label=label, definition=definition, strict_fused=s_fused, strict_pairs=s_pairs, fast_fused=f_fused, fast_pairs=f_pairs,
                     finite=bool(all(np.isfinite(b[0]).all() for b in ref)), strict_equal=[], first_diff=None, rmse=[], max=[], time_rel=[], digest=[])
            for k, ((so, to, do), (ss, ts, ds), (sf, tf, df)) in enumerate(zip(ref, strict, fast)):
                same = bool(np.array_equal(ss.view(np.uint8), so.view(np.uint8)) and real(ts) == real(to) and real(ds) == real(do))
                r["strict_equal"].append(same)
                if not same and r["first_diff"] is None:
                    where = np.argwhere((ss.view(np.uint8) != so.view(np.uint8)).reshape(gc.ROWS, gc.COLS, -1).any(axis=2))
                    y, x = (int(v) for v in where[0]) if len(where) else (-1, -1)
                    r["first_diff"] = dict(batch=k, differing_cells=int(len(where)), y=y, x=x, engine=[float(v) for v in ss[y, x]], oracle=[float(v) for v in so[y, x]],
                                           t=[float(ts), float(to)], dt=[float(ds), float(do)])
                err = np.maximum(0.0, sf[..., 0].astype(np.float64) - bed) - np.maximum(0.0, so[..., 0].astype(np.float64) - bed)
                r["rmse"].append(float(np.sqrt(np.mean(err ** 2))))
                r["max"].append(float(np.abs(err).max()))
                r["time_rel"].append(abs(float(tf) - float(to)) / max(1.0, abs(float(to))))
                r["digest"].append(hashlib.sha1(sf.tobytes() + np.array([tf, df], np.float64).tobytes()).hexdigest())
            results.append(r)
    with open(out_file, "w") as f:
        json.dump(results, f)
    bad = [r["label"] for r in results if not all(r["strict_equal"])]
    print(f"{path} {precision}: {len(results)} cases, STRICT parts from the oracle on {len(bad)} {bad[:4]}, FAST depth RMSE up to {max(max(r['rmse']) for r in results):.3e} m, "
          f"max {max(max(r['max']) for r in results):.3e} m, time {max(max(r['time_rel']) for r in results):.3e}", flush=True)


if __name__ == "__main__":
    main(*sys.argv[1:5])
