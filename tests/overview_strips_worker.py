"""Worker of tests/test_gpu_overview.py::test_strips_gather_overview: WORLD strips as threads of this process on the one GPU (the
library's own strip loop over tests/fake_rccl, as zones_strips_worker.py).  Every rank aggregates its OWNED rows on its device --
blocks are anchored to the global grid, so a block that a strip border cuts comes in two parts --, which is what
StripRunner.gather_overview does on each rank; the parts are put together by the function gather_overview uses
(strips.assemble_overviews; the transport between the ranks, torch.distributed there, is a list here) and compared with the single
domain's overviews, bit for bit.  The factors do not divide the strips' heights.
usage: overview_strips_worker.py <world>"""
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
os.environ["HIPIMS_MI_NO_TORCH"] = "1"
os.environ["GPU_MAX_HW_QUEUES"] = "24"          # every rank's streams on hardware queues of their own (strip_threads_worker.py)
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
from hipims_mi import strips, synthetic as syn  # noqa: E402

world = int(sys.argv[1])
cols, rows, batches, dx = 257, 130, [3, 4, 5], 2.5
names = ["depth", "maxdepth", "fsl", "maxfsl", "dischargex", "dischargey", "velocityx", "velocityy", "froude"]
pairs = [(n, k) for n in names for k in ("max", "min", "count")]
requests = [(16, np.float64), (3, np.float64), (100, np.float32), (1, np.float32)]
g = strips.ghost_rows(hp.SCHEME_GODUNOV)
st, bed, man = syn.s_rough(cols, rows)
parts = strips.partition(rows, world, g)
assert all((own_hi - own_lo) % f for own_lo, own_hi, _, _ in parts for f, _ in requests if f > 1)


def overviews(dom, row0, nrows):
    return [(dom.overview_shape(f, row0, nrows)[0], dom.overview([n for n, _ in pairs], [k for _, k in pairs], f, dtype=t, row0=row0, nrows=nrows))
            for f, t in requests]


single = hp.Domain(cols, rows, dx=dx)
single.upload(st, bed, man); single.set_target_time(1e9)
single.update_timestep()
for n in batches:
    single.step_batch(n)
want = overviews(single, 0, rows)
single.close()

lib = hp.load_library()
hp._check(lib, lib.hp_comm_load(os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so").encode()), "hp_comm_load")
uid = hp.comm_unique_id()
mine, errors = [None] * world, []
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
        for n in batches:
            dom.strip_step_batch(n)
        mine[r] = overviews(dom, own_lo - lo, own_hi - own_lo)          # the ghost rows belong to the neighbours
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
same, live = True, True
for k, (factor, dtype) in enumerate(requests):
    got = strips.assemble_overviews([mine[r][k] for r in range(world)], [kind for _, kind in pairs])
    assert want[k][0] == 0
    u = np.uint64 if dtype == np.float64 else np.uint32
    for (name, kind), a, b in zip(pairs, got, want[k][1]):
        if not (a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))):
            same = False
            print("differs:", factor, name, kind, a.shape, b.shape, flush=True)
    depth_max = got[pairs.index(("depth", "max"))]
    live = live and bool((depth_max > 0).any() and got[pairs.index(("velocityx", "count"))].sum() > 0)
print("ranks", world, "overviews identical in every bit", same, "water in the picture", live, flush=True)
os._exit(0 if same and live else 1)
