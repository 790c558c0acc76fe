"""What a zone-recorder sample costs a run, on one GPU: the wall time of ITER iterations of the benchmark's S-DAM domain
(4096^2 fp64, levels 10 | 1 m) in batches of BATCH, for these ways of getting per-zone volume / flooded-area series out of it:
  none      nothing is recorded (the floor)
  blocks    Domain.zones_sample() after every batch, 64 rectangular zones (8 x 8)
  one       ... one zone over the whole grid (the non-blocking mass-balance series)
  random    ... independent random ids 0..64 per cell: every wave mixed, the documented worst case
  download  Domain.download() of the whole state after every batch (537 MB): the only way without the recorder
Every wall figure is host time from the first step_batch to the end of a final sync, median [min, max] of REPS runs from the
same saved state (state_save / state_restore), after one untimed run.  For every id layout the sample alone (one fill + hp::
record_zones) is also timed between two events on the domain's stream, KERNEL_REPS samples back to back, next to the existing
statistics pass on the same state in the same process (Domain.stats(): hp::domain_stats, its one-block fold and a 56-byte copy),
which reads 40 of the same 42 bytes per cell.
usage: python tools/zones_stage_timing.py [--mode none|blocks|one|random|download|all] [--reps 5] [--size 4096] [--iterations 200] [--batch 20]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
from hipims_mi import synthetic as syn  # noqa: E402

KERNEL_REPS = 20


def zone_raster(mode, n):
    y, x = np.mgrid[0:n, 0:n]
    if mode == "blocks":
        return (1 + (y * 8 // n) * 8 + (x * 8 // n)).astype(np.uint16), 64
    if mode == "one":
        return np.ones((n, n), np.uint16), 1
    return np.random.default_rng(1).integers(0, 65, (n, n)).astype(np.uint16), 64


def one_run(dom, mode, iterations, batch):
    dom.state_restore()
    dom.sync()
    t0 = time.perf_counter()
    for _ in range(iterations // batch):
        dom.step_batch(batch)
        if mode in ("blocks", "one", "random"):
            dom.zones_sample()
        elif mode == "download":
            dom.download()
    dom.sync()
    return (time.perf_counter() - t0) * 1e3


def sample_alone(dom):
    """ms per sample (fill + kernel) and ms per Domain.stats() (kernel + fold + copy), both between two stream events"""
    dom.sync()
    dom.zones_sample(); dom.stats()                        # untimed
    per_sample, per_stats = [], []
    for _ in range(5):
        dom.timer_start()
        for _ in range(KERNEL_REPS):
            dom.zones_sample()
        per_sample.append(dom.timer_stop() / KERNEL_REPS)
        dom.timer_start()
        dom.stats()
        per_stats.append(dom.timer_stop())
    return statistics.median(per_sample), statistics.median(per_stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--batch", type=int, default=20)
    args = ap.parse_args()
    n = args.size
    print(f"# {hp.device_info(0)['name']}; tools/zones_stage_timing.py --mode {args.mode} --reps {args.reps} --size {n} "
          f"--iterations {args.iterations} --batch {args.batch}; library {os.environ.get('HIPIMS_MI_LIB', hp.LIB_PATH)}", flush=True)
    st, bed, man = syn.s_dam(n, n, dtype=np.float64, levels=(10.0, 1.0))
    dom = hp.Domain(n, n)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.step_batch(120)                                   # the benchmark's window: 120 iterations in
    dom.state_save()
    modes = ["none", "blocks", "one", "random", "download"] if args.mode == "all" else [args.mode]
    for mode in modes:
        recording = mode in ("blocks", "one", "random")
        if recording:
            ids, zone_count = zone_raster(mode, n)
            dom.zones_enable(ids, zone_count, capacity=4096)
        one_run(dom, mode, args.iterations, args.batch)   # untimed
        times = [one_run(dom, mode, args.iterations, args.batch) for _ in range(args.reps)]
        extra = ""
        if recording:
            per_sample, per_stats = sample_alone(dom)
            extra = (f" | {zone_count} zones, {8 * dom.zones_info()['stride']} B per record; one sample {per_sample * 1e3:.1f} us, "
                     f"Domain.stats() {per_stats * 1e3:.1f} us on the same state: ratio {per_sample / per_stats:.2f}")
            dom.zones_disable()
        print(f"{mode:8s} {n}x{n} f64 S-DAM, {args.iterations} iterations in batches of {args.batch}: "
              f"{statistics.median(times):.2f} [{min(times):.2f}, {max(times):.2f}] ms wall ({args.reps} runs){extra}", flush=True)
    dom.close()


if __name__ == "__main__":
    main()
