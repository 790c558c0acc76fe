"""What a picture of a run costs, on one GPU: the benchmark's S-DAM domain (4096^2 fp64, levels 10 | 1 m, 120 iterations in), same
process, same state, for two value sets -- depth alone; depth, velocityx, velocityy and froude -- and two ways of getting them:
  derive    Domain.derive(values): the full rasters (hp::derive_rasters, 8 bytes per cell and value over the host link)
  overview  Domain.overview(values, "max", factor) at factors 4, 16 and 64 (hp::overview_blocks + hp::overview_finish, 8 bytes per
            BLOCK and value over the host link)
End to end: host wall time of the call, which ends with the device synchronised and the arrays on the host; median [min, max] of
REPS calls after an untimed one.  The kernels alone: `--kernel-only N` queues N calls of every configuration in the order it
prints and nothing else -- the run to put under `rocprofv3 --kernel-trace --stats`; `--trace FILE` then reads that run's kernel
trace (CSV) and prints the median time of every configuration's kernels per call, dispatch by dispatch in the same order.  Bytes per call
of both kernels: cells x 40 read; derive_rasters writes cells x 8 per value on top, overview_blocks nothing of that order.
usage: python tools/overview_stage_timing.py [--reps 7] [--size 4096] [--kernel-only N] [--trace kernel_trace.csv --per N]"""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]

SETS = {"depth": ["depth"], "depth+velocity+froude": ["depth", "velocityx", "velocityy", "froude"]}
FACTORS = (4, 16, 64)


def configurations():
    for tag, values in SETS.items():
        yield tag, values, None
        for factor in FACTORS:
            yield tag, values, factor


def read_trace(path, per):
    """Median kernel time of every configuration from a rocprofv3 kernel trace of a `--kernel-only per` run."""
    rows = list(csv.DictReader(open(path, newline="")))
    name = next(k for k in rows[0] if k.lower() == "kernel_name")
    t0, t1 = (next(k for k in rows[0] if k.lower() == key) for key in ("start_timestamp", "end_timestamp"))
    rows.sort(key=lambda r: int(r[t0]))
    ours = [(r[name], (int(r[t1]) - int(r[t0])) / 1e3) for r in rows if "derive_rasters" in r[name] or "overview_" in r[name]]
    at = 0
    for tag, values, factor in configurations():
        if factor is None:                                # (rasters above the scratch cap take several launches a call: summed per call)
            end = at
            while end < len(ours) and "derive_rasters" in ours[end][0]:
                end += 1
            launches = (end - at) // per
            assert launches >= 1 and launches * per == end - at, (at, end, per)
            times = {f"derive_rasters ({launches} a call)": [sum(t for _, t in ours[at + k * launches:at + (k + 1) * launches]) for k in range(per)]}
            at = end
        else:
            times = {"overview_blocks": [], "overview_finish": []}
            for _ in range(per):
                for k in times:
                    assert k in ours[at][0], (at, k, ours[at])
                    times[k].append(ours[at][1])
                    at += 1
        what = "derive" if factor is None else f"overview factor {factor}"
        print(f"{tag:22s} {what:20s} | " + ", ".join(f"{k} {statistics.median(v):.1f} us [{min(v):.1f}, {max(v):.1f}]" for k, v in times.items())
              + f" ({per} calls)", flush=True)
    assert at == len(ours), (at, len(ours))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--kernel-only", type=int, default=0)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--per", type=int, default=10)
    args = ap.parse_args()
    if args.trace:
        return read_trace(args.trace, args.per)
    import numpy as np
    import hipims_mi as hp
    from hipims_mi import synthetic as syn
    n = args.size
    st, bed, man = syn.s_dam(n, n, dtype=np.float64, levels=(10.0, 1.0))
    dom = hp.Domain(n, n)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.step_batch(120)                                   # the benchmark's window: 120 iterations in
    dom.sync()
    call = lambda values, factor: dom.derive(values) if factor is None else dom.overview(values, "max", factor)
    if args.kernel_only:
        for tag, values, factor in configurations():
            for _ in range(args.kernel_only):
                call(values, factor)
        dom.close()
        return
    print(f"# {hp.device_info(0)['name']}; tools/overview_stage_timing.py --reps {args.reps} --size {n}; {n}x{n} f64 S-DAM; "
          f"ms per call, host wall, median [min, max] of {args.reps} after an untimed one", flush=True)
    for tag, values, factor in configurations():
        call(values, factor)                              # untimed (first-use allocations, page faults of fresh arrays)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = call(values, factor)
            times.append((time.perf_counter() - t0) * 1e3)
        arrays = list(out.values()) if isinstance(out, dict) else out
        what = "derive" if factor is None else f"overview factor {factor}"
        print(f"{tag:22s} {what:20s} | {statistics.median(times):8.3f} [{min(times):.3f}, {max(times):.3f}] ms | "
              f"{sum(a.nbytes for a in arrays) / 1e6:.3f} MB to the host", flush=True)
    dom.close()


if __name__ == "__main__":
    main()
