"""What a probe-recorder sample costs a run, on one GPU: the wall time of ITER iterations of the benchmark's S-DAM domain
(4096^2 fp64, levels 10 | 1 m) in batches of BATCH, for three ways of getting a hydrograph out of it:
  none      nothing is recorded (the floor)
  probes    Domain.probes_sample() after every batch: 64 gauges and 8 sections of 4096 cells (4 along rows, 4 along columns)
  download  Domain.download() of the whole state after every batch (537 MB): the only way without the recorder
Every figure is host wall time from the first step_batch to the end of a final sync, median [min, max] of REPS runs from the
same saved state (state_save / state_restore), after one untimed run.  `none` and `download` use nothing the recorder added, so
HIPIMS_MI_LIB may point them at an older library for an A/B run.  Under `rocprofv3 --kernel-trace --stats -- python
tools/probes_stage_timing.py --mode probes --reps 1` the trace gives hp::record_probes' own time.
usage: python tools/probes_stage_timing.py [--mode none|probes|download|all] [--reps 5] [--size 4096] [--iterations 200] [--batch 20]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
from hipims_mi import frontend, synthetic as syn  # noqa: E402


def probe_set(n):
    rng = np.random.default_rng(1)
    gauges = list(zip(rng.integers(1, n - 1, 64).tolist(), rng.integers(1, n - 1, 64).tolist()))
    at = [n // 5, 2 * n // 5, 3 * n // 5, 4 * n // 5]
    sections = [frontend.rasterise_section((0, y), (n - 1, y)) for y in at] + [frontend.rasterise_section((x, 0), (x, n - 1)) for x in at]
    return gauges, sections


def one_run(dom, mode, iterations, batch):
    dom.state_restore()
    dom.sync()
    t0 = time.perf_counter()
    for _ in range(iterations // batch):
        dom.step_batch(batch)
        if mode == "probes":
            dom.probes_sample()
        elif mode == "download":
            dom.download()
    dom.sync()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--batch", type=int, default=20)
    args = ap.parse_args()
    n = args.size
    print(f"# {hp.device_info(0)['name']}; tools/probes_stage_timing.py --mode {args.mode} --reps {args.reps} --size {n} "
          f"--iterations {args.iterations} --batch {args.batch}; library {os.environ.get('HIPIMS_MI_LIB', hp.LIB_PATH)}", flush=True)
    st, bed, man = syn.s_dam(n, n, dtype=np.float64, levels=(10.0, 1.0))
    dom = hp.Domain(n, n)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.step_batch(120)                                   # the benchmark's window: 120 iterations in
    dom.state_save()
    modes = ["none", "probes", "download"] if args.mode == "all" else [args.mode]
    for mode in modes:
        if mode == "probes":
            gauges, sections = probe_set(n)
            dom.probes_enable(gauges, sections, capacity=4096)
        one_run(dom, mode, args.iterations, args.batch)   # untimed
        times = [one_run(dom, mode, args.iterations, args.batch) for _ in range(args.reps)]
        extra = ""
        if mode == "probes":
            info = dom.probes_info()
            cells = len(gauges) + sum(len(s.cells) for s in sections)
            extra = (f" | {len(gauges)} gauges, {len(sections)} sections of {len(sections[0].cells)} cells: {cells} cells x 40 B gathered, "
                     f"{8 * info['stride']} B written per sample")
            dom.probes_disable()
        print(f"{mode:8s} {n}x{n} f64 S-DAM, {args.iterations} iterations in batches of {args.batch}: "
              f"{statistics.median(times):.2f} [{min(times):.2f}, {max(times):.2f}] ms wall ({args.reps} runs){extra}", flush=True)
    dom.close()


if __name__ == "__main__":
    main()
