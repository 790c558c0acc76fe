"""Worker of tests/test_gpu_sparse.py::test_strips_gather_sparse: WORLD strips as threads of this process on the one GPU (the
library's own strip loop over tests/fake_rccl, as overview_strips_worker.py).  Every rank compacts its OWNED rows on its device,
which is what StripRunner.gather_sparse does on each rank; the parts are concatenated in rank order by the function gather_sparse
uses (frontend.combine_sparse; the transport between the ranks, torch.distributed there, is a list here) and compared with the
single domain's results, word for word.
usage: sparse_strips_worker.py <world>"""
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
cols, rows, batches, dx = 257, 130, [3, 4, 5], 2.5
names = ["depth", "maxdepth", "fsl", "maxfsl", "dischargex", "dischargey", "velocityx", "velocityy", "froude"]
requests = [(names, "depth", 0.01, np.float64), (names, "dischargex", -np.inf, np.float32), (["froude", "depth"], "froude", 0.5, np.float64),
            (["depth"], "depth", 1e9, np.float32)]
g = strips.ghost_rows(hp.SCHEME_GODUNOV)
st, bed, man = syn.s_rough(cols, rows)
parts = strips.partition(rows, world, g)


def results(dom, row0, nrows):
    return [dom.sparse(values, select=select, above=above, dtype=t, row0=row0, nrows=nrows) for values, select, above, t in requests]


single = hp.Domain(cols, rows, dx=dx)
single.upload(st, bed, man); single.set_target_time(1e9)
single.update_timestep()
for n in batches:
    single.step_batch(n)
want = results(single, 0, rows)
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
        mine[r] = results(dom, own_lo - lo, own_hi - own_lo)          # the ghost rows belong to the neighbours
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
for k, (values, select, above, dtype) in enumerate(requests):
    got = frontend.combine_sparse([mine[r][k] for r in range(world)])
    ok = (got[0].dtype == want[k][0].dtype and np.array_equal(got[0], want[k][0]) and got[1].dtype == want[k][1].dtype and np.array_equal(got[1], want[k][1])
          and all(a.dtype == b.dtype == np.dtype(dtype) and a.tobytes() == b.tobytes() for a, b in zip(got[2], want[k][2])))
    if not ok:
        same = False
        print("differs:", values, select, above, got[0][-1], want[k][0][-1], flush=True)
depth = frontend.combine_sparse([mine[r][0] for r in range(world)])
live = 0 < int(depth[0][-1]) <= rows * cols and int(want[1][0][-1]) == rows * cols and int(want[3][0][-1]) == 0
print("ranks", world, "sparse results identical in every word", same, "water selected", live, flush=True)
os._exit(0 if same and live else 1)
