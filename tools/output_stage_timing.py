"""Time per output of the two output paths on one GPU, same process, same state (S-ROUGH after a developing batch):
  A  the host path : Domain.download() + frontend.derive_output per target (what Model.write_outputs did before derive existed)
  B  the device path: Domain.derive(targets) -- one call, rasters only over the host link
for 4096^2 fp64, 8192^2 fp32 and 16384 x 8192 fp64 and for 1, 5 (the example model's target count) and 9 rasters: median of
REPS runs after a warm-up; both paths end with the device synchronised (download / derive sync before they return).
`--kernel-only N` runs N derive calls of nine rasters on 4096^2 fp64 and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats -- python tools/output_stage_timing.py --kernel-only 10` for the kernel's own time
(bytes per call: cells x (40 + 8 x 9)).
usage: python tools/output_stage_timing.py [--reps 5] [--cases 4096x4096:f64,...] [--kernel-only N]"""
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

TARGETS = {1: ["depth"], 5: ["depth", "velocityx", "velocityy", "fsl", "maxdepth"],
           9: ["depth", "maxdepth", "fsl", "maxfsl", "dischargex", "dischargey", "velocityx", "velocityy", "froude"]}


def make(cols, rows, precision, steps=200):
    real = np.float64 if precision == "f64" else np.float32
    st, bed, man = syn.s_rough(cols, rows, dtype=real)
    dom = hp.Domain(cols, rows, precision=precision)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.step_batch(steps)
    dom.sync()
    return dom, bed


def median_ms(f, reps):
    f()                                                  # warm-up (first-use allocations, page faults of fresh arrays)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="4096x4096:f64,8192x8192:f32,16384x8192:f64")
    ap.add_argument("--counts", default="1,5,9")
    ap.add_argument("--kernel-only", type=int, default=0)
    args = ap.parse_args()
    if args.kernel_only:
        dom, _ = make(4096, 4096, "f64", steps=50)
        for _ in range(args.kernel_only):
            dom.derive(TARGETS[9])
        dom.close()
        return
    print(f"# {hp.device_info(0)['name']}; median [min, max] ms per output over {args.reps} runs after a warm-up")
    print("# grid precision rasters | A: download + derive_output (of which download) | B: derive | A / B")
    for case in args.cases.split(","):
        shape, precision = case.split(":")
        cols, rows = (int(v) for v in shape.split("x"))
        dom, bed = make(cols, rows, precision)
        dl = median_ms(lambda: dom.download(), args.reps)
        for k in (int(v) for v in args.counts.split(",")):
            names = TARGETS[k]

            def host():
                state = dom.download()
                return [frontend.derive_output(n, state, bed, 1.0) for n in names]

            a = median_ms(host, args.reps)
            b = median_ms(lambda: dom.derive(names), args.reps)
            print(f"{cols}x{rows} {precision} {k} | {a[0]:9.1f} [{a[1]:.1f}, {a[2]:.1f}] ({dl[0]:.1f}) | {b[0]:9.1f} [{b[1]:.1f}, {b[2]:.1f}] | {a[0] / b[0]:5.2f}",
                  flush=True)
        dom.close()


if __name__ == "__main__":
    main()
