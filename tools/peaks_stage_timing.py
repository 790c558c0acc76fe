"""Device time of one peak-tracker sample (Domain.peaks_sample, all five values on) on one GPU, 4096^2 fp64, for three states:
  S-DAM    the benchmark's window (bench.py: S-DAM levels 10 | 1 m, 120 iterations in -- more than 99 % still water, all of it wet)
  S-ROUGH  after 200 iterations (moving water over a rough wet/dry bed)
  dry      the S-ROUGH bed without water
Every figure is the HIP-event time of ONE sample (hp_timer_start / hp_timer_stop around the launch), median [min, max] of REPS
samples with a batch of 8 iterations in front of each, after a first sample that turns NODATA into values.  Algorithmic bytes of
the last timed sample: 40 B per cell + 8 B read per wet cell and enabled value + 8 B per value that changed (counted from the
accumulators before and after).  `--derive N` adds N Domain.derive calls of one raster on the S-ROUGH state, so that the same
run under `rocprofv3 --kernel-trace --stats -- python tools/peaks_stage_timing.py --derive 5` gives hp::derive_rasters' and
hp::track_peaks' kernel times side by side (derive: 48 B per cell).  `--model` times a Model run of the example model
directory with and without peak targets (wall time, a sample after every batch).
usage: python tools/peaks_stage_timing.py [--reps 5] [--size 4096] [--derive N] [--model]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
from hipims_mi import synthetic as syn  # noqa: E402

NAMES = list(hp.PEAK_CODES)


def states(n):
    st, bed, man = syn.s_dam(n, n, dtype=np.float64, levels=(10.0, 1.0))
    yield "S-DAM", st, bed, man, 120
    st, bed, man = syn.s_rough(n, n, dtype=np.float64)
    yield "S-ROUGH", st, bed, man, 200
    dry = st.copy()
    dry[..., 0] = bed; dry[..., 1] = bed; dry[..., 2:] = 0.0
    yield "dry", dry, bed, man, 0


def one_case(name, st, bed, man, steps, reps, derive_calls):
    n = bed.shape[0]
    dom = hp.Domain(n, n)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    if steps:
        dom.step_batch(steps)
    dom.peaks_enable(NAMES)
    dom.sync()
    dom.timer_start(); dom.peaks_sample(); first = dom.timer_stop()
    times, before = [], None
    for k in range(reps):
        dom.step_batch(8)
        if k == reps - 1:
            before = dom.peaks()
        dom.sync()
        dom.timer_start(); dom.peaks_sample(); times.append(dom.timer_stop())
    after = dom.peaks()
    changed = sum(int((before[v] != after[v]).sum()) for v in NAMES)
    wet = dom.stats()["cells_wet"]
    cells = n * n
    bytes_ = 40 * cells + 8 * len(NAMES) * wet + 8 * changed
    med = statistics.median(times)
    print(f"{name:8s} {n}x{n} f64 | first sample {first:.4f} ms | sample {med:.4f} [{min(times):.4f}, {max(times):.4f}] ms | "
          f"wet cells {wet} of {cells}, values changed by the last sample {changed} | "
          f"{bytes_ / 1e6:.1f} MB -> {bytes_ / (times[-1] * 1e-3) / 1e12:.2f} TB/s (last sample, {times[-1]:.4f} ms)", flush=True)
    if derive_calls and name == "S-ROUGH":
        for _ in range(derive_calls):
            dom.derive(["depth"])
    dom.close()


def model_runs():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from hipims_mi.model import Model
    from model_dir import make_newcastle
    for tag, peaks in (("warm-up", None), ("without peak targets", None), ("with five peak targets", NAMES), ("without peak targets", None),
                       ("with five peak targets", NAMES)):
        with tempfile.TemporaryDirectory() as tmp:
            m = Model(make_newcastle(tmp, duration=1800, frequency=600), output_format=".npy", peaks=peaks)
            m.scheme.automatic_queue = False
            m.scheme.queue_addition_size = 64
            t0 = time.perf_counter()
            m.run()
            wall = time.perf_counter() - t0
            print(f"Model, example directory (342x195, 1800 s, batches of 64, {m.scheme.iterations} iterations, "
                  f"{m.scheme.iterations // 64} batches) {tag}: {wall:.3f} s", flush=True)
            m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--derive", type=int, default=0)
    ap.add_argument("--model", action="store_true")
    args = ap.parse_args()
    print(f"# {hp.device_info(0)['name']}; tools/peaks_stage_timing.py --reps {args.reps} --size {args.size}", flush=True)
    for case in states(args.size):
        one_case(*case, args.reps, args.derive)
    if args.model:
        model_runs()


if __name__ == "__main__":
    main()
