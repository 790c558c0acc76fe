"""Worker of tests/test_gpu_bed_shapes.py::test_strips: WORLD strips as threads of this process on the one GPU (the library's own
strip loop over tests/fake_rccl, as zones_strips_worker.py).  Every rank adds every shape with GLOBAL ids and applies between
batches, which is what StripRunner.bed_shape_add / bed_apply do on each rank; the owned rows of state and bed, put together as
gather_owned / gather_bed do (the transport between the ranks, torch.distributed there, is a list here), are compared with the
single domain's after every round.  The cut rows run through shape A (the wall spans all rows).
usage: bed_strips_worker.py <world> <reaches: 1 | 2 | 2odd>"""
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd"), os.path.join(ROOT, "tests")]
os.environ["HIPIMS_MI_NO_TORCH"] = "1"
os.environ["GPU_MAX_HW_QUEUES"] = "24"          # every rank's streams on hardware queues of their own (strip_threads_worker.py)
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
from hipims_mi import strips  # noqa: E402
import bed_shapes_worker as W  # noqa: E402

world, mode = int(sys.argv[1]), sys.argv[2]
reaches = 1 if mode == "1" else 2
batches = {"1": [7, 8, 7, 8, 7, 8], "2": [8, 8, 8, 8, 8, 8], "2odd": [7, 1, 8, 8]}[mode]
g = strips.ghost_rows(hp.SCHEME_GODUNOV) * reaches
st, bed, man = W.arrays()
parts = strips.partition(W.ROWS, world, g)

single = W.make("godunov-fast-f64")
W.add_shapes(single)
want = []
for k, n in enumerate(batches):
    single.step_batch(n)
    if not (mode == "2odd" and k == 0):                   # (the strips' refused apply is no apply)
        single.bed_apply()
    want.append((single.download(), single.download(hp.ARRAY_BED)))
single.close()

lib = hp.load_library()
hp._check(lib, lib.hp_comm_load(os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so").encode()), "hp_comm_load")
uid = hp.comm_unique_id()
got, refused, errors = [[None] * world for _ in batches], [None] * world, []
tickets = [None] * world
start = threading.Barrier(world)


def rank_main(r):
    try:
        own_lo, own_hi, lo, hi = parts[r]
        dom = hp.Domain(W.COLS, hi - lo, dx=W.DX, global_rows=W.ROWS, row_offset=lo, ghost_rows=g if reaches > 1 else 0)
        dom.upload(st[lo:hi], bed[lo:hi], man[lo:hi])
        dom.strip_comm_init(uid, r, world)
        dom.set_time(W.T0)
        dom.set_target_time(1e9)
        tickets[r] = dom.strip_peer_ticket()
        start.wait()
        dom.strip_peer_connect(tickets, r)
        start.wait()
        dom.strip_update_timestep()
        W.add_shapes(dom)                                  # global ids: the library keeps this strip's rows, ghost rows included
        for k, n in enumerate(batches):
            dom.strip_step_batch(n)
            if mode == "2odd" and k == 0:                  # two reaches after an odd batch: refused on the ranks whose ghost rows are short
                rc = lib.hp_bed_apply(dom.h)
                refused[r] = (rc, lib.hp_last_error().decode() if rc else "")
            else:
                dom.bed_apply()
            local, local_bed = dom.download(), dom.download(hp.ARRAY_BED)
            got[k][r] = (local[own_lo - lo:own_hi - lo].copy(), local_bed[own_lo - lo:own_hi - lo].copy())
            start.wait()                                   # (peer-written ghost rows: nobody runs ahead into the next batch while a neighbour reads)
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
same = []
for k in range(len(batches)):
    state = np.concatenate([p[0] for p in got[k]], axis=0)
    zb = np.concatenate([p[1] for p in got[k]], axis=0)
    same.append(bool(np.array_equal(state, want[k][0]) and np.array_equal(zb, want[k][1])))
moved = bool((want[-1][1] != bed).any())
ok = all(same) and moved
if mode == "2odd":
    # every rank of a world > 1 has an interior side: all of them are short after 7 iterations
    ok = ok and all(rc == -5 and "even batch" in text for rc, text in refused)
print("ranks", world, "mode", mode, "state and bed identical in every round", same, "the bed moved", moved, "refused", refused, flush=True)
os._exit(0 if ok else 1)
