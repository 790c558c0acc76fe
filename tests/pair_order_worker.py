"""Worker of tests/test_gpu_pair_order.py (HP_PAIR_ORDER, HP_TWO_STEP, HP_PAIR_SKIP and HP_MARCH2_RSEG are read once per process): FAST fp64
runs on the two grids of that test; writes, per grid, the final state, the time-control scalars, the launch counts and what
hp_pair_stats said after every batch (out[9] skipped rows, out[11] tiles run out of tile-row order) to an .npz.
usage: pair_order_worker.py <case> <out.npz>
  dam         S-DAM as bench.py runs it (closed edge ring: the ring's column groups and the first and last tile rows march as well),
              on a third, wider grid too, where still column groups lie between the dam's and the ring's
  dam_open    the same two pools with the edge ring at its pool's level: only the column group with the dam marches
  edge_front  one level with a step inside the last column group only
  still       one level, the edge ring included: nothing marches
  rough       S-ROUGH: every column group marches
  interleave  dam_open in batches of 1, 2, 7 and 8 with a checkpoint, its restore and a partial upload between them
  fixed       dam_open with a fixed timestep"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
import hipims_mi as hp  # noqa: E402
from hipims_mi import synthetic as syn  # noqa: E402

case, out = sys.argv[1:3]
GRIDS = ((722, 130), (482, 75))      # 12 windows in 3 groups; 8 windows in 2 groups, 73 updated rows (bands of 10: tiles of 8 and 2 rows)
if case == "dam":
    GRIDS += ((1262, 75),)           # 21 windows in 6 groups: the dam's group and the ring's two march, three stand between them


def pools(cols, rows, step_col, levels):
    """Flat bed, two levels meeting at step_col, the edge ring at the level of its side (no wall)."""
    st = np.zeros((rows, cols, 4))
    st[:, :step_col, 0] = levels[0]
    st[:, step_col:, 0] = levels[1]
    st[..., 1] = st[..., 0]
    return st, np.zeros((rows, cols)), np.full((rows, cols), 0.03)


def scene(cols, rows):
    if case == "dam":
        return syn.s_dam(cols, rows)
    if case in ("dam_open", "interleave", "fixed"):
        return pools(cols, rows, cols // 2, (10.0, 1.0))
    if case == "edge_front":
        return pools(cols, rows, cols - 82, (1.0, 1.5))
    if case == "still":
        return pools(cols, rows, cols // 2, (1.0, 1.0))
    if case == "rough":
        return syn.s_rough(cols, rows)
    raise SystemExit(f"unknown case {case}")


result = {}
for cols, rows in GRIDS:
    st, bed, man = scene(cols, rows)
    kw = dict(dynamic_dt=False, dt_fixed=0.02) if case == "fixed" else {}
    dom = hp.Domain(cols, rows, precision="f64", **kw)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    moved, skipped = [], []

    def batch(n):
        dom.step_batch(n)
        ps = dom.pair_stats()
        moved.append(int(ps["reordered_tiles"]))
        skipped.append(int(ps["skipped_rows"]))

    if case != "interleave":
        for n in (8, 8, 8, 8, 8):                                 # 40 iterations
            batch(n)
    else:
        for n in (8, 1, 2, 7):
            batch(n)
        dom.state_save()
        for n in (8, 7, 2):
            batch(n)
        dom.state_restore()
        for n in (1, 8, 8):
            batch(n)
        r0 = rows // 2 - 4                                        # a mound in the first column group, which stood still so far
        part = dom.download(row0=r0, nrows=8)
        part[2:6, 40:44, 0] += 0.5
        part[2:6, 40:44, 1] = part[2:6, 40:44, 0]
        dom.upload_rows(part, r0)
        for n in (2, 8, 7, 1, 8):
            batch(n)
    sc = dom.read_scalars()
    counts = dom.launch_counts()
    key = f"{cols}x{rows}"
    result[key + "_state"] = dom.download()
    result[key + "_scalars"] = np.array([sc["time"], sc["timestep"]], np.float64)
    result[key + "_counts"] = np.array([sc["iterations"], counts[0], counts[1]], np.int64)
    result[key + "_moved"] = np.array(moved, np.int64)
    result[key + "_skipped"] = np.array(skipped, np.int64)
    dom.close()
    print(f"{case} {key}: t = {sc['time']!r}, iterations {sc['iterations']}, launches {counts}, reordered tiles per batch {moved}, "
          f"skipped rows per batch {skipped}")
np.savez(out, **result)
