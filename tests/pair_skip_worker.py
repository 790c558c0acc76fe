"""Worker of tests/test_gpu_pair_skip.py (HP_TWO_STEP and HP_PAIR_SKIP are read once per process): a FAST fp64 run on a grid that is
a multiple neither of the pair kernel's 60 columns nor of its tile height; writes the final state, the time-control scalars and the
rows the pair launches skipped (hp_pair_stats out[9], read after every batch) to an .npz.
usage: pair_skip_worker.py <case> <out.npz>
  dam         S-DAM: the front moves into still water, the west and east pools are skipped meanwhile
  dam_fixed   the same with a fixed timestep
  fronts      one still lake with small mounds beside window and tile boundaries and on tile corners: fronts enter skipped tiles from
              every side and diagonally
  ulp         still lakes side by side whose levels, or beds, differ by one ulp, a mound far away
  zmax        a still lake whose Zmax lies below Z in patches (raised at the first step, skipped afterwards)
  negzero     discharges of -0.0 in a still lake (dynamic timestep)
  negzero_fixed  the same with a fixed timestep
  disabled    disabled cells (-9999) in a still lake
  interleave  a checkpoint restored mid-run, a partial upload that drops a mound into a tile the launch before skipped, batches of odd
              length, downloads between batches, a target time that shortens and then zeroes a step"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
import hipims_mi as hp  # noqa: E402
from hipims_mi import synthetic as syn  # noqa: E402

case, out = sys.argv[1:3]
cols, rows = 1031, 707
rng = np.random.default_rng(11)


def lake(level=1.0):
    st, bed, man = syn.s_dam(cols, rows, levels=(level, level))
    return st, bed, man


def mound(st, r, c, dz=0.4, k=2):
    st[r - k:r + k + 1, c - k:c + k + 1, 0] += dz
    st[r - k:r + k + 1, c - k:c + k + 1, 1] = st[r - k:r + k + 1, c - k:c + k + 1, 0]


if case.startswith("dam"):
    st, bed, man = syn.s_dam(cols, rows)
elif case == "fronts":
    st, bed, man = lake()
    for r, c in ((100, 181), (100, 300), (250, 420), (252, 541), (400, 660), (400, 781), (560, 120), (600, 900), (60, 960)):
        mound(st, r, c)
    for r, c in ((330, 240), (480, 360)):                     # (a corner of four windows)
        mound(st, r, c, k=0)
elif case == "ulp":
    st, bed, man = lake()
    st[:, 300:480, 0] = np.nextafter(1.0, 2.0)                # one ulp above the lake beside it
    bed[:, 600:780] = np.nextafter(0.0, 1.0)                  # one ulp of bed under the same level
    st[200:400, 840:960, 0] = np.nextafter(1.0, 0.0)
    st[..., 1] = np.maximum(st[..., 1], st[..., 0])
    mound(st, 650, 60)
elif case == "zmax":
    st, bed, man = lake()
    st[100:300, 200:500, 1] = 0.5
    st[400:420, 700:1000, 1] = np.nextafter(1.0, 0.0)
    mound(st, 600, 100)
elif case.startswith("negzero"):
    st, bed, man = lake()
    st[100:300, 200:500, 2] = -0.0
    st[350:360, 100:1000, 3] = -0.0
    st[500:520, 600:620, 2:] = -0.0
    mound(st, 650, 900)
elif case == "disabled":
    st, bed, man = lake()
    st[200, 300, 1] = -9999.0
    st[400:403, 610:613, 0] = -9999.0
    st[500, 121, 1] = -9999.0
    mound(st, 100, 900)
elif case == "interleave":
    st, bed, man = syn.s_dam(cols, rows)
else:
    raise SystemExit(f"unknown case {case}")
man[:, 700:] = rng.uniform(0.01, 0.05, (rows, cols - 700))   # (a Manning array over part of the grid)

kw = dict(dynamic_dt=False, dt_fixed=0.02) if case.endswith("fixed") else {}
dom = hp.Domain(cols, rows, precision="f64", **kw)
dom.upload(st, bed, man)
dom.set_target_time(1e9)
skipped = []


def batch(n):
    dom.step_batch(n)
    ps = dom.pair_stats()
    skipped.append(int(ps["skipped_rows"]) if ps else 0)


if case != "interleave":
    for n in (40, 7, 64, 1, 30, 100, 58):
        batch(n)
else:
    batch(40)
    dom.state_save()
    batch(41)
    dom.download()
    batch(30)
    dom.state_restore()
    batch(30)
    batch(24)
    # a mound dropped into the east pool, far from the front: rows the launch before skipped
    part = dom.download(row0=380, nrows=20)
    part[5:10, 820:825, 0] += 0.5
    part[5:10, 820:825, 1] = part[5:10, 820:825, 0]
    dom.upload_rows(part, 380)
    batch(31)
    batch(20)
    sc = dom.read_scalars()
    dom.set_target_time(sc["time"] + 2.5 * sc["timestep"])   # a step shortened to the target, then steps of zero length
    batch(9)
    dom.set_target_time(1e9)
    batch(50)
final = dom.download()
sc = dom.read_scalars()
counts = dom.launch_counts()
np.savez(out, state=final, t=sc["time"], dt=sc["timestep"], iterations=sc["iterations"], launches=counts[0],
         skipped=np.array(skipped, np.int64))
dom.close()
print(f"{case}: t = {sc['time']!r}, iterations {sc['iterations']}, flux launches {counts[0]}, skipped rows per batch {skipped}")
