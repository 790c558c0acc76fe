"""Worker of tests/test_gpu_zones.py::test_strips_gather_zones: WORLD strips as threads of this process on the one GPU (the
library's own strip loop over tests/fake_rccl, as probes_strips_worker.py).  Every rank records its local rows with the ghost
rows' ids set to 0 -- a sample after every batch, nothing exchanged --, which is what StripRunner.zones_enable / zones_sample do
on each rank; the parts are put together by the function gather_zones uses (frontend.combine_zones; the transport between the
ranks, torch.distributed there, is a list here) and compared with the single domain's records, word for word.
usage: zones_strips_worker.py <world>"""
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
cols, rows, batches, dx, flood = 257, 130, [3, 4, 5, 2, 1, 8], 2.5, 0.1
g = strips.ghost_rows(hp.SCHEME_GODUNOV)
st, bed, man = syn.s_rough(cols, rows)
parts = strips.partition(rows, world, g)
# zones that straddle every cut (columns), zones cut along rows that are no strip borders, and random ids in one corner
y, x = np.mgrid[0:rows, 0:cols]
ids = 1 + (x * 3 // cols) + 3 * (y * 4 // rows)
ids[:40, :50] = np.random.default_rng(1).integers(0, 14, (40, 50))
zone_count = 13

single = hp.Domain(cols, rows, dx=dx)
single.upload(st, bed, man); single.set_target_time(1e9)
single.update_timestep()
single.zones_enable(ids, zone_count, flood_depth=flood)
for n in batches:
    single.step_batch(n)
    single.zones_sample()
want = single.zone_records()
single.close()

lib = hp.load_library()
hp._check(lib, lib.hp_comm_load(os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so").encode()), "hp_comm_load")
uid = hp.comm_unique_id()
records, errors = [None] * world, []
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
        local = ids[lo:hi].copy()
        local[:own_lo - lo] = 0                           # the ghost rows belong to the neighbours
        local[own_hi - lo:] = 0
        dom.zones_enable(local, zone_count, flood_depth=flood, capacity=4)         # (a small buffer: drained along the way)
        for n in batches:
            dom.strip_step_batch(n)
            dom.zones_sample()
        records[r] = dom.zone_records()
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
got = frontend.combine_zones(records)
same = got.dtype == want.dtype and got.shape == want.shape and bool(np.array_equal(got, want))
series = hp.split_zone_records(got, zone_count, dx)
live = bool((series["wet"] > 0).all() and (series["volume"] > 0).all() and len(series["t"]) == len(batches))
print("ranks", world, "zones identical in every word", same, "every zone carries water", live, flush=True)
os._exit(0 if same and live else 1)
