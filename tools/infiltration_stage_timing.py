"""What the infiltration costs, on one GPU: the 4096^2 fp64 S-DAM domain, 200 single iterations (HP_TWO_STEP=0, set here before
the library loads: a domain with an infiltration never runs pairs, so the run without it is held to single iterations too) with
  none       no infiltration: the baseline of the same run (on a library without hp_boundary_add_infiltration only this leg runs)
  pervious   every cell of class 1: the pass reads the class byte, half a state entry, the bed and F of every cell and writes the level
             and F where the soil takes water up (the whole wet grid)
  class 0    every cell impervious: the pass reads the class bytes and nothing else
The infiltration costs one launch of bdy_infiltration per iteration and takes the area boundaries out of the flux kernel (none
here).  Every figure is taken REPS times after an untimed pass, host wall time that ends with the device synchronised, given as
median [min, max] and per iteration; the last column is the difference to the baseline's median per iteration.
usage: python tools/infiltration_stage_timing.py [--reps 3] [--size 4096] [--iterations 200]"""
import argparse
import os
import statistics
import sys
import time

os.environ["HP_TWO_STEP"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import hipims_mi as hp
    from hipims_mi import synthetic as syn
    n = args.size
    st, bed, man = syn.s_dam(n, n, dtype=np.float64, levels=(10.0, 1.0))
    have = hasattr(hp.Domain, "add_infiltration")
    print(f"# {hp.device_info(0)['name']}; tools/infiltration_stage_timing.py --reps {args.reps} --size {n}; {n}x{n} f64 S-DAM, HP_TWO_STEP=0; "
          f"{args.iterations} iterations in one batch; median [min, max] of {args.reps} after an untimed pass", flush=True)
    base = None
    for leg in ("none", "pervious", "class 0") if have else ("none",):
        dom = hp.Domain(n, n)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        dom.update_timestep()
        if leg != "none":
            dom.add_infiltration(np.full((n, n), 1 if leg == "pervious" else 0, np.uint8), [dict(ks=1e-5, suction=0.1, deficit=0.3)])
        dom.step_batch(120)                               # the benchmark's window: 120 iterations in
        dom.sync()
        times = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            dom.step_batch(args.iterations)
            dom.sync()
            if rep:
                times.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(times)
        base = med if base is None else base
        taken = float(dom.infiltration_read().max()) if leg != "none" else 0.0
        print(f"{leg:>9s} | {med:9.3f} [{min(times):.3f}, {max(times):.3f}] ms | {med / args.iterations * 1e3:8.2f} us per iteration | "
              f"{(med - base) / args.iterations * 1e3:+8.2f} us against none | largest F: {taken:.6f} m | pairs: {dom.pair_stats()['pairs']}", flush=True)
        dom.close()


if __name__ == "__main__":
    main()
