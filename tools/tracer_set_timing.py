"""What a tracer set costs against that many single tracers, on one GPU: the 4096^2 fp64 S-DAM domain, 200 single iterations
(HP_TWO_STEP=0, set here before the library loads: a domain with a tracer never runs pairs, so the run without it is held to
single iterations too) with
  none         no tracer: the baseline
  single       hp_tracer_enable: tracer_step, the kernel a set of K is to be measured against (K runs of it, K runs of the water)
  set K        hp_tracer_enable_set of K = 1, 2, 4, 8 species without decay: tracer_step_set, the face solves once per cell
  set K decay  the same with lambda = 1e-3 / s on every species: one more division per cell and species
Every leg has a domain of its own, all in one process; M = 1 everywhere.  The legs are timed in turn, REPS rounds over all of them
after an untimed round, host wall time that ends with the device synchronised.  Per leg: the median [min, max], the median per
iteration, its cost over `none` per iteration, and for a set that cost over K times the single tracer's cost: below 1 the set is
cheaper than K tracers on one run of the water, and K runs of the water come on top of that for the single tracer.
usage: python tools/tracer_set_timing.py [--reps 3] [--size 4096] [--iterations 200]"""
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
    if args.reps < 3:
        ap.error("at least three repetitions")
    import numpy as np
    import hipims_mi as hp
    from hipims_mi import synthetic as syn
    n = args.size
    st, bed, man = syn.s_dam(n, n, dtype=np.float64, levels=(10.0, 1.0))
    print(f"# {hp.device_info(0)['name']}; tools/tracer_set_timing.py --reps {args.reps} --size {n}; {n}x{n} f64 S-DAM, HP_TWO_STEP=0; "
          f"{args.iterations} iterations in one batch; legs interleaved, median [min, max] of {args.reps} rounds after an untimed one", flush=True)
    legs = [("none", 0, 0.0), ("single", 0, 0.0)] + [(f"set {k}" + (" decay" if lam else ""), k, lam) for k in (1, 2, 4, 8) for lam in (0.0, 1e-3)]
    ones = np.ones((n, n))
    doms = {}
    for name, k, lam in legs:
        dom = doms[name] = hp.Domain(n, n)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        dom.update_timestep()
        if name == "single":
            dom.tracer_enable(ones)
        elif k:
            dom.tracer_enable_set(species=k, decay=[lam] * k)
            for s in range(k):
                dom.tracer_write(ones, species=s)
        dom.step_batch(120)                               # the benchmark's window: 120 iterations in
        dom.sync()
    times = {name: [] for name, _, _ in legs}
    for rep in range(args.reps + 1):
        for name, _, _ in legs:
            dom = doms[name]
            t0 = time.perf_counter()
            dom.step_batch(args.iterations)
            dom.sync()
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e3)
    per = {name: statistics.median(t) / args.iterations * 1e3 for name, t in times.items()}     # us per iteration
    single = per["single"] - per["none"]
    for name, k, lam in legs:
        t = times[name]
        cost = per[name] - per["none"]
        ratio = f"{cost / (k * single):6.3f} of {k} x single" if k and single > 0 else " " * 20
        total = float(sum(doms[name].tracer_read(species=s).sum() for s in range(max(k, 1)))) if name != "none" else 0.0
        print(f"{name:>11s} | {statistics.median(t):9.3f} [{min(t):.3f}, {max(t):.3f}] ms | {per[name]:8.2f} us per iteration | "
              f"{cost:+8.2f} us against none | {ratio} | sum(M): {total:.6f} | pairs: {doms[name].pair_stats()['pairs']}", flush=True)
    for dom in doms.values():
        dom.close()


if __name__ == "__main__":
    main()
