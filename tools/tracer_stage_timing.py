"""What the tracer costs, on one GPU: the 4096^2 fp64 S-DAM domain, 200 single iterations (HP_TWO_STEP=0, set here before the
library loads: a domain with a tracer never runs pairs, so the run without it is held to single iterations too) with
  none       no tracer: the baseline of the same run (on a library without hp_tracer_enable only this leg runs)
  traced     the tracer on every cell (M = 1 everywhere): tracer_step reads the state, the bed and M of every cell and its four
             neighbours, makes four exact face solves a cell and writes M
  dry        the tracer on a dry domain (the levels on the bed): every cell is a copy case, the kernel reads the state and the bed,
             solves no face and copies M
The tracer costs one launch of tracer_step per iteration.  Every figure is taken REPS times after an untimed pass, host wall time
that ends with the device synchronised, given as median [min, max] and per iteration; the last column is the difference to the
baseline's median per iteration.
  dry none   the dry domain without the tracer: the dry leg's own baseline (the flux kernel skips dry rows, so the wet baseline is
             not the one to subtract)
usage: python tools/tracer_stage_timing.py [--reps 3] [--size 4096] [--iterations 200]"""
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
    have = hasattr(hp.Domain, "tracer_enable")
    print(f"# {hp.device_info(0)['name']}; tools/tracer_stage_timing.py --reps {args.reps} --size {n}; {n}x{n} f64 S-DAM, HP_TWO_STEP=0; "
          f"{args.iterations} iterations in one batch; median [min, max] of {args.reps} after an untimed pass", flush=True)
    base = None
    for leg in ("none", "traced", "dry", "dry none") if have else ("none",):
        dom = hp.Domain(n, n)
        if leg.startswith("dry"):
            dry = st.copy()
            dry[..., 0] = dry[..., 1] = bed
            dom.upload(dry, bed, man)
        else:
            dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        dom.update_timestep()
        if leg in ("traced", "dry"):
            dom.tracer_enable(np.ones((n, n)))
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
        total = float(dom.tracer_read().sum()) if leg in ("traced", "dry") else 0.0
        print(f"{leg:>9s} | {med:9.3f} [{min(times):.3f}, {max(times):.3f}] ms | {med / args.iterations * 1e3:8.2f} us per iteration | "
              f"{(med - base) / args.iterations * 1e3:+8.2f} us against none | sum(M): {total:.6f} | pairs: {dom.pair_stats()['pairs']}", flush=True)
        dom.close()


if __name__ == "__main__":
    main()
