"""What a tracer set's exchange with the bed costs, on one GPU: the 4096^2 fp64 S-DAM domain, 200 single iterations (HP_TWO_STEP=0,
set here before the library loads: a domain with a tracer never runs pairs) with sets of K = 1, 4 and 8 species and, for each K,
  plain   no species exchanges: tracer_step_set<T, false>, the kernel of the set before the exchange
  all     every species exchanges (settling 1e-3 m/s below 0.5 N/m2, erosion 1e-4 units/(m2 s) above 2 N/m2): tracer_step_set<T, true>
  one     species 0 alone exchanges: the other species take the uniform branch round D
Every leg has a domain of its own, all in one process; M = 1 and D = 0.5 everywhere.  The legs are timed in turn, REPS rounds over
all of them after an untimed round, host wall time that ends with the device synchronised.  Per leg: the median [min, max], the median
per iteration, and what it adds per iteration to the plain set of the same K, with the larger of the two legs' spreads (max - min, per
iteration) beside it.
--legs plain times the plain legs alone: with HIPIMS_MI_LIB naming a library built from the commit before the exchange, that is the
same set on the parent, to hold this build's plain legs against (the calls of the exchange are not made).
usage: python tools/tracer_exchange_timing.py [--reps 5] [--size 4096] [--iterations 200] [--legs all|plain]"""
import argparse
import os
import statistics
import sys
import time

os.environ["HP_TWO_STEP"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
EXCHANGE = dict(settling=1e-3, tau_deposit=0.5, tau_erode=2.0, erodibility=1e-4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--legs", choices=("all", "plain"), default="all")
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("at least three repetitions")
    import numpy as np
    import hipims_mi as hp
    from hipims_mi import synthetic as syn
    n = args.size
    st, bed, man = syn.s_dam(n, n, dtype=np.float64, levels=(10.0, 1.0))
    print(f"# {hp.device_info(0)['name']}; tools/tracer_exchange_timing.py --reps {args.reps} --size {n} --legs {args.legs}; library "
          f"{os.environ.get('HIPIMS_MI_LIB') or 'of this tree'}; {n}x{n} f64 S-DAM, HP_TWO_STEP=0; {args.iterations} iterations in one batch; "
          f"legs interleaved, median [min, max] of {args.reps} rounds after an untimed one", flush=True)
    kinds = ("plain",) if args.legs == "plain" else ("plain", "all", "one")
    legs = [(f"set {k} {kind}", k, kind) for k in (1, 4, 8) for kind in kinds]
    ones = np.ones((n, n))
    doms = {}
    for name, k, kind in legs:
        dom = doms[name] = hp.Domain(n, n)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        dom.update_timestep()
        dom.tracer_enable_set(species=k)
        for s in range(k):
            dom.tracer_write(ones, species=s)
            if kind == "all" or (kind == "one" and s == 0):
                dom.tracer_set_exchange(s, deposit=0.5 * ones, **EXCHANGE)
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
    spread = {name: (max(t) - min(t)) / args.iterations * 1e3 for name, t in times.items()}
    for name, k, kind in legs:
        t = times[name]
        plain = f"set {k} plain"
        added = f"{per[name] - per[plain]:+8.2f} us against plain (spread {max(spread[name], spread[plain]):.2f})" if kind != "plain" else " " * 40
        dom = doms[name]
        M = float(sum(dom.tracer_read(species=s).sum() for s in range(k)))
        D = float(sum(dom.tracer_deposit_read(species=s).sum() for s in range(k if kind == "all" else 1))) if kind != "plain" else 0.0
        print(f"{name:>11s} | {statistics.median(t):9.3f} [{min(t):.3f}, {max(t):.3f}] ms | {per[name]:8.2f} us per iteration | {added} | "
              f"sum(M): {M:.6f} | sum(D): {D:.6f} | pairs: {dom.pair_stats()['pairs']}", flush=True)
    for dom in doms.values():
        dom.close()


if __name__ == "__main__":
    main()
