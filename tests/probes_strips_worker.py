"""Worker of tests/test_gpu_probes.py::test_strips_gather_probes: WORLD strips as threads of this process on the one GPU (the
library's own strip loop over tests/fake_rccl, as peaks_strips_worker.py).  Every rank records the points on the rows it OWNS
as gauges -- a sample after every batch, nothing exchanged --, which is what StripRunner.probes_enable / probes_sample do on
each rank (strips.probe_points); the parts are put together by the function gather_probes uses (strips.assemble_probes; the
transport between the ranks, torch.distributed there, is a list here) and compared with the single domain's record.
usage: probes_strips_worker.py <world>"""
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
os.environ["HIPIMS_MI_NO_TORCH"] = "1"
os.environ["GPU_MAX_HW_QUEUES"] = "24"          # every rank's streams on hardware queues of their own (strip_threads_worker.py)
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
from hipims_mi import frontend, strips, synthetic as syn  # noqa: E402

world = int(sys.argv[1])
cols, rows, batches, dx = 67, 45, [3, 4, 5, 2, 1, 8], 2.5
g = strips.ghost_rows(hp.SCHEME_GODUNOV)
st, bed, man = syn.s_rough(cols, rows)
parts = strips.partition(rows, world, g)
cuts = [p[1] for p in parts[:-1]]
# gauges on the owned rows next to each cut (both sides), sections that cross every cut (one walked north, one south-west)
gauge_xy = [(x, y) for c in cuts for x, y in ((5, c - 1), (40, c), (61, c - 1), (20, c))]
sections = [frontend.rasterise_section((2, 1), (64, 43)), frontend.rasterise_section((50, 44), (9, 0)),
            frontend.rasterise_section((33, 2), (33, 42))]
assert all(s.cells[:, 1].min() < min(cuts) and s.cells[:, 1].max() >= max(cuts) for s in sections)

single = hp.Domain(cols, rows, dx=dx)
single.upload(st, bed, man); single.set_target_time(1e9)
single.update_timestep()
single.probes_enable(gauge_xy, sections)
for n in batches:
    single.step_batch(n)
    single.probes_sample()
want = single.probes()
single.close()

lib = hp.load_library()
hp._check(lib, lib.hp_comm_load(os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so").encode()), "hp_comm_load")
uid = hp.comm_unique_id()
gauges, secs, points = strips.probe_points(gauge_xy, sections)
series, errors = [None] * world, []
tickets = [None] * world
start = threading.Barrier(world)


def rank_main(r):
    try:
        own_lo, own_hi, lo, hi = parts[r]
        dom = hp.Domain(cols, hi - lo, dx=dx, global_rows=rows, row_offset=lo)
        dom.upload(st[lo:hi], bed[lo:hi], man[lo:hi])
        dom.strip_comm_init(uid, r, world)
        dom.set_target_time(1e9)
        tickets[r] = dom.strip_peer_ticket()
        start.wait()
        dom.strip_peer_connect(tickets, r)
        start.wait()
        dom.strip_update_timestep()
        mine = np.flatnonzero((points[:, 1] >= own_lo) & (points[:, 1] < own_hi))
        dom.probes_enable(points[mine] - np.array([0, lo]), (), capacity=4)        # (a small buffer: drained along the way)
        for n in batches:
            dom.strip_step_batch(n)
            dom.probes_sample()
        got = dom.probes()
        series[r] = (mine, got["t"], got["gauges"])
        dom.strip_comm_destroy()
        dom.close()
    except Exception as e:                                # noqa: BLE001
        errors.append((r, repr(e)))
        try:
            start.abort()
        except Exception:                                 # noqa: BLE001
            pass


threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
for t in threads:
    t.start()
for t in threads:
    t.join(300)
if errors or any(t.is_alive() for t in threads):
    print("FAILED", errors, [t.is_alive() for t in threads], flush=True); os._exit(2)
got = strips.assemble_probes(series, gauges, secs, dx)
same = all(got[k].shape == want[k].shape and np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)) for k in ("t", "gauges", "sections"))
live = bool((want["sections"] != 0).any(axis=0).all() and (want["gauges"] != -9999.0).any() and len(want["t"]) == len(batches))
print("ranks", world, "probes bit-identical", same, "every section carries water", live, flush=True)
os._exit(0 if same and live else 1)
