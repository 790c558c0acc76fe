"""What a moving bed costs, on one GPU: the 4096^2 fp64 S-DAM domain with a 4096-cell breach (one column of cells, base 0 m to
-0.5 m over the run), 200 iterations in batches of 20, in three forms:
  (a) plain    no applies
  (b) apply    Domain.bed_apply() behind every batch (hp::bed_apply over the listed cells + one device copy of the state)
  (c) round    the host round trip an apply replaces, behind every batch: sync, read the time, download state and bed,
               frontend.BedShapes.apply, upload the bed, upload the state -- the only way before hp_bed_apply: the yardstick
and bed_apply alone (kernel + copy, bracketed with the domain's event timer on the idle stream).  Every figure is taken REPS times
after an untimed pass and given as median [min, max]; (a)-(c) are host wall times that end with the device synchronised.
usage: python tools/bed_stage_timing.py [--reps 3] [--size 4096] [--round-reps 3]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--batch", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import hipims_mi as hp
    from hipims_mi import frontend, synthetic as syn
    n = args.size
    st, bed, man = syn.s_dam(n, n, dtype=np.float64, levels=(10.0, 1.0))
    cells = [y * n + n // 2 for y in range(1, min(n - 1, 4097))][:4096]
    series = [(0.0, 0.0), (1e4, 1.0)]                     # moving through the whole run: every apply changes every listed cell
    fmt = lambda v: f"{statistics.median(v):9.3f} [{min(v):.3f}, {max(v):.3f}] ms"
    print(f"# {hp.device_info(0)['name']}; tools/bed_stage_timing.py --reps {args.reps} --size {n}; {n}x{n} f64 S-DAM, {len(cells)}-cell breach; "
          f"{args.iterations} iterations in batches of {args.batch}; median [min, max] of {args.reps} after an untimed pass", flush=True)

    def fresh(with_shape):
        dom = hp.Domain(n, n)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        dom.update_timestep()
        if with_shape:
            dom.bed_shape_add(cells, -0.5, series)
        dom.step_batch(120)                               # the benchmark's window: 120 iterations in
        dom.sync()
        return dom

    def timed(dom, behind_batch):
        times = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            for _ in range(args.iterations // args.batch):
                dom.step_batch(args.batch)
                behind_batch()
            dom.sync()
            if rep:
                times.append((time.perf_counter() - t0) * 1e3)
        return times

    dom = fresh(False)
    print(f"(a) plain  | {fmt(timed(dom, lambda: None))}", flush=True)
    dom.close()
    dom = fresh(True)
    print(f"(b) apply  | {fmt(timed(dom, dom.bed_apply))}", flush=True)
    alone = []
    for rep in range(args.reps + 1):
        dom.sync()
        dom.timer_start()
        dom.bed_apply()
        ms = dom.timer_stop()
        if rep:
            alone.append(ms)
    print(f"bed_apply alone (kernel + state copy) | {fmt(alone)} | changed by the last one: {dom.bed_info()['changed_last']}", flush=True)
    dom.close()
    dom = fresh(False)
    ref = frontend.BedShapes(n, n)
    ref.add(cells, -0.5, series, bed=bed)

    def round_trip():
        dom.sync()
        t = dom.read_scalars()["time"]
        s, zb = dom.download(), dom.download(hp.ARRAY_BED)
        ref.apply(s, zb, t)
        dom.upload(bed=zb)
        dom.upload(state=s)
    print(f"(c) round  | {fmt(timed(dom, round_trip))}", flush=True)
    dom.close()


if __name__ == "__main__":
    main()
