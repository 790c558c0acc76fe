"""Worker of tests/test_gpu_still_pairs.py (HP_TWO_STEP is read once per process): still water on the FAST fp64 engine; writes the
final state and the time-control scalars to an .npz.
usage: still_pairs_worker.py <variant> <out.npz>
  dynamic  a dam break beside still water -- lakes at rest at one level and at another behind a wall, a lake over a bed step, Zmax
           below Z, a disabled cell, a tiny discharge, discharges of -0.0, a Manning array
  fixed    the same with a fixed timestep, without the -0.0 discharges (LAB_NOTES R7.2: with them the parent's pairs and single
           iterations already differ)
  fixed_negzero  the same with them (tools/diag_negzero_fixed.py)
  lake     one deep lake at rest over the whole grid, Zmax below Z in a patch, a Manning array: every wavefront is a still run, so
           the still runs alone price the timestep"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
import hipims_mi as hp  # noqa: E402
from hipims_mi import synthetic as syn  # noqa: E402

variant, out = sys.argv[1:3]
cols, rows = 1030, 700
rng = np.random.default_rng(7)
if variant == "lake":
    st = np.zeros((rows, cols, 4))
    st[..., 0] = 1.0
    bed = np.full((rows, cols), -40.0)
    man = rng.uniform(0.01, 0.05, (rows, cols))
    st[..., 1] = st[..., 0]
    st[200:500, 300:800, 1] = 0.25
else:
    st, bed, man = syn.s_dam(cols, rows)              # Z = 10 m west of the middle, 1 m east, flat bed, walls
    st[:, :, 2:] = 0.0
    # a wall (a dry ridge) across the east pool, and behind it a lake at another level
    bed[450, 520:1029] = 6.0
    st[450, 520:1029, 0] = 6.0
    st[451:699, 520:1029, 0] = 2.5
    # a lake over a bed step: one level, two beds
    bed[100:300, 900:1000] = 0.5
    # Zmax below Z, a disabled cell, a tiny discharge, discharges of -0.0
    st[:, :, 1] = st[:, :, 0]
    st[500:600, 600:900, 1] = st[500:600, 600:900, 0] - 0.5
    st[620, 700, 1] = -9999.0
    st[640, 750, 2] = 1e-12
    if variant != "fixed":
        st[660:680, 600:1000, 2] = -0.0
        st[300:320, 600:1000, 3] = -0.0
    # a Manning array over part of the east pool
    man[:, 700:] = rng.uniform(0.01, 0.05, (rows, cols - 700))
kw = dict(dynamic_dt=False, dt_fixed=0.02) if variant.startswith("fixed") else {}
dom = hp.Domain(cols, rows, precision="f64", **kw)
dom.upload(st, bed, man)
dom.set_target_time(1e9)
for n in (40, 7, 64, 1, 30):
    dom.step_batch(n)
final = dom.download()
sc = dom.read_scalars()
counts = dom.launch_counts()
np.savez(out, state=final, t=sc["time"], dt=sc["timestep"], iterations=sc["iterations"], launches=counts[0])
dom.close()
print(f"{variant}: t = {sc['time']!r}, iterations {sc['iterations']}, flux launches {counts[0]}")
