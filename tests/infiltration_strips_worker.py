"""Worker of tests/test_gpu_infiltration.py::test_strips: WORLD strips as threads of this process on the one GPU (the library's own
strip loop over tests/fake_rccl, as links_strips_worker.py), one reach of ghost rows, an exchange after every iteration.  Every rank
adds the rain and then the infiltration with the rows of the global soil raster that it stores, ghost rows included, which is what
StripRunner.add_infiltration does on each rank.  The owned rows of the state and of F -- what StripRunner.gather_infiltration puts
together -- are compared with the single domain's after every batch; so are the ghost rows' F with their owners'.
usage: infiltration_strips_worker.py <world>"""
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
import test_infiltration as TI  # noqa: E402
import test_links as T  # noqa: E402

world = int(sys.argv[1])
batches = [8, 12, 20]                                  # 40 iterations
g = strips.ghost_rows(hp.SCHEME_GODUNOV)
st, bed, man, soil = TI.soil_scene()
parts = strips.partition(T.ROWS, world, g)


def prepare(dom, lo, hi):
    dom.set_target_time(1e9)
    dom.add_uniform(T.RAIN["definition"], T.RAIN["series"], T.RAIN["interval"], T.RAIN["length"])
    dom.add_infiltration(soil[lo:hi], TI.CLASSES)


single = hp.Domain(T.COLS, T.ROWS, dx=T.DX)
single.upload(st, bed, man)
prepare(single, 0, T.ROWS)
single.update_timestep()
want = []
for n in batches:
    single.step_batch(n)
    want.append((single.download(), single.infiltration_read()))
single.close()

lib = hp.load_library()
hp._check(lib, lib.hp_comm_load(os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so").encode()), "hp_comm_load")
uid = hp.comm_unique_id()
got, errors = [[None] * world for _ in batches], []
tickets = [None] * world
start = threading.Barrier(world)


def rank_main(r):
    try:
        own_lo, own_hi, lo, hi = parts[r]
        dom = hp.Domain(T.COLS, hi - lo, dx=T.DX, global_rows=T.ROWS, row_offset=lo)
        dom.upload(st[lo:hi], bed[lo:hi], man[lo:hi])
        dom.strip_comm_init(uid, r, world)
        tickets[r] = dom.strip_peer_ticket()
        start.wait()
        dom.strip_peer_connect(tickets, r)
        start.wait()
        prepare(dom, lo, hi)
        dom.strip_update_timestep()
        for k, n in enumerate(batches):
            dom.strip_step_batch(n)
            local, F = dom.download(), dom.infiltration_read()
            got[k][r] = (local[own_lo - lo:own_hi - lo].copy(), F[own_lo - lo:own_hi - lo].copy(), bool(np.array_equal(F, want[k][1][lo:hi])))
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
same_state, same_f, same_ghosts = [], [], []
for k in range(len(batches)):
    same_state.append(bool(np.array_equal(np.concatenate([p[0] for p in got[k]], axis=0), want[k][0])))
    same_f.append(bool(np.array_equal(np.concatenate([p[1] for p in got[k]], axis=0), want[k][1])))
    same_ghosts.append(all(p[2] for p in got[k]))
taken = float(want[-1][1].sum())
ok = all(same_state) and all(same_f) and all(same_ghosts) and taken > 0.01
print("world", world, "state identical", same_state, "F identical", same_f, "ghost rows' F their owners'", same_ghosts, "infiltrated depth summed", taken, flush=True)
print("the strips are the single domain True" if ok else "FAILED", flush=True)
os._exit(0 if ok else 1)
