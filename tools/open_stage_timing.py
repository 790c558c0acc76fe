"""What the open boundary costs, on one GPU: the 4096^2 fp64 S-DAM domain, 200 single iterations (HP_TWO_STEP=0, set here before the
library loads: a domain with an open boundary never runs pairs, so the run without it is held to single iterations too) with
  0      no open boundary: what the parent commit runs (on a library without hp_boundary_add_open only this leg runs: the yardstick)
  1      the whole east edge open (4094 ring cells, one segment)
  4      all four edges open (16376 ring cells, four segments, one call)
The opened ring cells get a real bed, the one of their inward neighbours, in every leg, so all three legs run on the same arrays.  An open
boundary costs one launch of 64-lane blocks over its ring cells per iteration, prices the edge ring anew on every iteration and takes
the area boundaries out of the flux kernel (none here).  Every figure is taken REPS times after an untimed pass, host wall time that
ends with the device synchronised, given as median [min, max] and per iteration.
usage: python tools/open_stage_timing.py [--reps 3] [--size 4096] [--iterations 200]"""
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
    for ring, inner in ((np.s_[0, 1:-1], np.s_[1, 1:-1]), (np.s_[-1, 1:-1], np.s_[-2, 1:-1]), (np.s_[1:-1, 0], np.s_[1:-1, 1]), (np.s_[1:-1, -1], np.s_[1:-1, -2])):
        bed[ring] = bed[inner]
        st[ring] = st[inner]
    have = hasattr(hp.Domain, "add_open")
    print(f"# {hp.device_info(0)['name']}; tools/open_stage_timing.py --reps {args.reps} --size {n}; {n}x{n} f64 S-DAM, HP_TWO_STEP=0; "
          f"{args.iterations} iterations in one batch; median [min, max] of {args.reps} after an untimed pass", flush=True)
    for edges in ((), ("east",), ("south", "north", "west", "east")) if have else ((),):
        dom = hp.Domain(n, n)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        dom.update_timestep()
        if edges:
            dom.add_open(list(edges))
            assert dom.open_info() == dict(segments=len(edges), cells=len(edges) * (n - 2))
        dom.step_batch(120)                               # the benchmark's window: 120 iterations in
        dom.sync()
        times = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            dom.step_batch(args.iterations)
            dom.sync()
            if rep:
                times.append((time.perf_counter() - t0) * 1e3)
        left = int((dom.open_read()["active"] > 0).sum()) if edges else 0
        print(f"{len(edges):2d} open edges | {statistics.median(times):9.3f} [{min(times):.3f}, {max(times):.3f}] ms | "
              f"{statistics.median(times) / args.iterations * 1e3:8.2f} us per iteration | cells water left through: {left} | pairs: {dom.pair_stats()['pairs']}", flush=True)
        dom.close()


if __name__ == "__main__":
    main()
