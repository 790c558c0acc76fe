"""What link groups cost, on one GPU: the 4096^2 fp64 S-DAM domain, 200 single iterations (HP_TWO_STEP=0, set here before the
library loads: a domain with links never runs pairs, so the run without links is held to single iterations too) with
  0      no link group: what the parent commit runs (on a library without hp_boundary_add_links only this leg runs: the yardstick)
  64     one group of 64 links across the dam line
  4096   one group of 4096 links across the dam line (one orifice per interior row, the last two on a second pair of columns)
Every link joins (cols/2 - 8, y) and (cols/2 + 8, y), or 16 columns further out on either side; a link group costs one 64-thread-block launch per iteration and takes the
area boundaries out of the flux kernel (none here).  Every figure is taken REPS times after an untimed pass, host wall time that
ends with the device synchronised, given as median [min, max] and per iteration.
usage: python tools/links_stage_timing.py [--reps 3] [--size 4096] [--iterations 200]"""
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
    have = hasattr(hp.Domain, "add_links")
    print(f"# {hp.device_info(0)['name']}; tools/links_stage_timing.py --reps {args.reps} --size {n}; {n}x{n} f64 S-DAM, HP_TWO_STEP=0; "
          f"{args.iterations} iterations in one batch; median [min, max] of {args.reps} after an untimed pass", flush=True)
    for count in (0, 64, 4096) if have else (0,):
        dom = hp.Domain(n, n)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        dom.update_timestep()
        if count:
            # exactly `count` links: the interior rows in turn (evenly spread while they last), a further pair of columns per pass over them
            per_pass = min(count, n - 2)
            rows = np.linspace(1, n - 2, per_pass).astype(int)
            dom.add_links([dict(a=(n // 2 - 8 - 16 * (k // per_pass), int(rows[k % per_pass])), b=(n // 2 + 8 + 16 * (k // per_pass), int(rows[k % per_pass])),
                                kind="orifice", level=0.0, size=0.5, coeff=0.6) for k in range(count)])
            assert dom.links_info()["links"] == count
        dom.step_batch(120)                               # the benchmark's window: 120 iterations in
        dom.sync()
        times = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            dom.step_batch(args.iterations)
            dom.sync()
            if rep:
                times.append((time.perf_counter() - t0) * 1e3)
        moved = int((dom.links_read()["active"] > 0).sum()) if count else 0
        print(f"{count:5d} links | {statistics.median(times):9.3f} [{min(times):.3f}, {max(times):.3f}] ms | "
              f"{statistics.median(times) / args.iterations * 1e3:8.2f} us per iteration | links that moved water: {moved} | pairs: {dom.pair_stats()['pairs']}", flush=True)
        dom.close()


if __name__ == "__main__":
    main()
