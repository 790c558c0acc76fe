"""What the selected cells of an output time cost, on one GPU: 4096^2 fp64, 120 iterations in, on two states -- the benchmark's
S-DAM (levels 10 | 1 m) and S-ROUGH (every tile live) -- for two value sets -- depth alone; depth, velocityx and velocityy -- and
two ways of getting them:
  derive  Domain.derive(values): the full rasters (hp::derive_rasters, 8 bytes per cell and value over the host link)
  sparse  Domain.sparse(values, select, above): the selected cells in CSR (hp::sparse_select, hp::sparse_scan_*, hp::sparse_scatter;
          8 bytes per ROW and 4 + 8 bytes per value per SELECTED cell over the host link), for depth above 0.01 m, for depth above
          the state's median wet depth, and for dischargex above -inf (every cell: more bytes than derive moves)
End to end: host wall time of the call, which ends with the device synchronised and the arrays on the host; median [min, max] of
REPS calls after an untimed one (Domain.sparse's untimed call counts, the timed ones make one library call each).  The kernels
alone: `--kernel-only N` queues N calls of every configuration in the order it prints and nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats`; `--trace FILE` then reads that run's kernel trace (CSV) and prints the median time of each of the
kernels, name by name.
usage: python tools/sparse_stage_timing.py [--reps 7] [--size 4096] [--kernel-only N] [--trace kernel_trace.csv]"""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]

SETS = {"depth": ["depth"], "depth+velocity": ["depth", "velocityx", "velocityy"]}
KERNELS = ("derive_rasters", "sparse_select", "sparse_scan_sums", "sparse_scan_top", "sparse_scan_offsets", "sparse_scatter")


def read_trace(path):
    """Median time of every kernel of this stage from a rocprofv3 kernel trace of a `--kernel-only` run."""
    rows = list(csv.DictReader(open(path, newline="")))
    name = next(k for k in rows[0] if k.lower() == "kernel_name")
    t0, t1 = (next(k for k in rows[0] if k.lower() == key) for key in ("start_timestamp", "end_timestamp"))
    for kernel in KERNELS:
        times = [(int(r[t1]) - int(r[t0])) / 1e3 for r in rows if kernel in r[name]]
        if times:
            print(f"{kernel:20s} | {statistics.median(times):8.1f} us [{min(times):.1f}, {max(times):.1f}] ({len(times)} launches)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--kernel-only", type=int, default=0)
    ap.add_argument("--trace", default=None)
    args = ap.parse_args()
    if args.trace:
        return read_trace(args.trace)
    import numpy as np
    import hipims_mi as hp
    from hipims_mi import synthetic as syn
    n = args.size
    if not args.kernel_only:
        print(f"# {hp.device_info(0)['name']}; tools/sparse_stage_timing.py --reps {args.reps} --size {n}; {n}x{n} f64; "
              f"ms per call, host wall, median [min, max] of {args.reps} after an untimed one", flush=True)
    for state_name, make in (("S-DAM", lambda: syn.s_dam(n, n, dtype=np.float64, levels=(10.0, 1.0))), ("S-ROUGH", lambda: syn.s_rough(n, n))):
        st, bed, man = make()
        dom = hp.Domain(n, n)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        dom.step_batch(120)                               # the benchmark's window: 120 iterations in
        dom.sync()
        depth = dom.derive("depth")["depth"]
        wet = depth[depth > 0.01]
        median = float(np.median(wet)) if len(wet) else 0.01
        del depth, wet
        selections = [None, ("depth", 0.01), ("depth", median), ("dischargex", -np.inf)]
        call = lambda values, sel: dom.derive(values) if sel is None else dom.sparse(values, sel[0], sel[1])
        for tag, values in SETS.items():
            for sel in selections:
                what = "derive" if sel is None else f"sparse {sel[0]} > {sel[1]:.4g}"
                if args.kernel_only:
                    for _ in range(args.kernel_only):
                        call(values, sel)
                    continue
                out = call(values, sel)                   # untimed (first-use allocations, page faults of fresh arrays, the counting call)
                times = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    out = call(values, sel)
                    times.append((time.perf_counter() - t0) * 1e3)
                if sel is None:
                    moved, share = sum(a.nbytes for a in out.values()), 1.0
                else:
                    moved, share = out[0].nbytes + out[1].nbytes + sum(a.nbytes for a in out[2]), len(out[1]) / (n * n)
                print(f"{state_name:8s} {tag:15s} {what:28s} | {statistics.median(times):8.3f} [{min(times):.3f}, {max(times):.3f}] ms | "
                      f"selected share {share:.4f} | {moved / 1e6:.3f} MB to the host", flush=True)
        dom.close()


if __name__ == "__main__":
    main()
