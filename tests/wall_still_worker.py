"""Worker of tests/test_gpu_wall_still.py (HP_TWO_STEP, HP_PAIR_SKIP, HP_PAIR_WALL and HP_MARCH2_RSEG are read once per process): one
FAST fp64 run in a small closed box; writes the final state, the time-control scalars and, read after every batch, what the last pair
launch skipped and recorded (hp_pair_stats out[9], hp_pair_wall_stats) to an .npz.
usage: wall_still_worker.py <case> <cols> <rows> <out.npz> [level bed [wall_bed]]
  lake        a still lake of the given level over the given bed inside the walls (a given wall_bed replaces the 9999.9 of the ring)
  dam         S-DAM: the front reaches the north and south walls at once and the west and east walls within the run
  wet_ring    one ring cell per side holds water at the lake's level on the lake's bed
  two_beds    the ring's bed is 9999.9 along one stretch of every side and 8888.8 along the rest
  disabled    one ring cell per side is disabled (-9999)
  negzero     cells beside the ring carry a discharge of -0.0
  upload      a row-range upload that changes nothing between batches
  upload_mound  a row-range upload that drops a mound beside the west wall
  bed_apply   a bed shape over a cell beside the south wall, applied between batches
  links       a link group whose ends lie beside the east and west walls, added between batches"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
import hipims_mi as hp  # noqa: E402
from hipims_mi import synthetic as syn  # noqa: E402

case, cols, rows, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
level, bed_level = (float(sys.argv[5]), float(sys.argv[6])) if len(sys.argv) > 6 else (1.0, 0.0)
wall_bed = float(sys.argv[7]) if len(sys.argv) > 7 else syn.WALL_BED

if case == "dam":
    st, bed, man = syn.s_dam(cols, rows)
else:
    st, bed, man = syn.s_dam(cols, rows, levels=(level, level))
    bed[1:-1, 1:-1] = bed_level
    for sl in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        bed[sl] = wall_bed
ring = ((0, cols // 3), (rows - 1, 2 * cols // 3), (rows // 3, 0), (2 * rows // 3, cols - 1))   # one cell per side, away from the corners
if case == "wet_ring":
    for r, c in ring:
        st[r, c, :2] = level
        bed[r, c] = bed_level
elif case == "two_beds":
    bed[0, cols // 4:] = 8888.8
    bed[-1, : cols // 2] = 8888.8
    bed[rows // 2:, 0] = 8888.8
    bed[: rows // 4, -1] = 8888.8
elif case == "disabled":
    for r, c in ring:
        st[r, c, 1] = -9999.0
elif case == "negzero":
    st[1, 3:9, 2] = -0.0
    st[rows // 2, 1, 3] = -0.0
    st[rows - 2, cols - 2, 2:] = -0.0

dom = hp.Domain(cols, rows, precision="f64")
dom.upload(st, bed, man)
dom.set_target_time(1e9)
skipped, wall_skipped, wall_still = [], [], []


def batch(n):
    dom.step_batch(n)
    skipped.append(int(dom.pair_stats()["skipped_rows"]))
    ws = dom.pair_wall_stats()
    wall_skipped.append(int(ws[0]))
    wall_still.append(int(ws[1]))


if case == "dam":
    # (1000 iterations at about a third of a cell each: the front has crossed the 270 cells to the walls of a box 542 wide)
    for n in (40, 7, 64, 1, 30, 58, 300, 500):
        batch(n)
else:
    batch(4)
    if case == "upload":
        dom.upload_rows(dom.download(row0=0, nrows=3), 0)
    elif case == "upload_mound":
        part = dom.download(row0=rows // 2, nrows=2)
        part[0, 1, 0] += 0.25
        part[0, 1, 1] = part[0, 1, 0]
        dom.upload_rows(part, rows // 2)
    elif case == "bed_apply":
        dom.bed_shape_add([(5, 1)], bed_level + 0.125, [(0.0, 1.0)])       # (x, y): beside the south wall; raised at once
        dom.bed_apply()
    elif case == "links":
        # a pump from beside the west wall to beside the east wall: single iterations while it is there, pairs again once it is gone
        dom.add_links([dict(a=(1, rows // 2), b=(cols - 2, rows // 2), kind=hp.LINK_PUMP, level=bed_level, size=0.5)])
        batch(3)
        dom.clear_boundaries()
    batch(3)
    batch(4)
    batch(1)
    if case in ("upload", "upload_mound", "bed_apply"):
        batch(8)                                   # (pairs in a row again: tiles away from the write are skipped as before it)
final = dom.download()
sc = dom.read_scalars()
counts = dom.launch_counts()
np.savez(out, state=final, t=sc["time"], dt=sc["timestep"], iterations=sc["iterations"], launches=counts[0],
         skipped=np.array(skipped, np.int64), wall_skipped=np.array(wall_skipped, np.int64), wall_still=np.array(wall_still, np.int64))
dom.close()
print(f"{case} {cols}x{rows}: t = {sc['time']!r}, iterations {sc['iterations']}, flux launches {counts[0]}, skipped {skipped}, "
      f"beside the ring: skipped {wall_skipped}, still {wall_still}")
