"""Worker of tests/test_gpu_links.py::test_strips: WORLD strips as threads of this process on the one GPU (the library's own strip
loop over tests/fake_rccl, as bed_strips_worker.py).  Every rank adds the rain and then every link with GLOBAL ids, which is what
StripRunner.add_links does on each rank; the links lie so that every strip stores both ends or neither, some are stored by two
strips (rows next to the cuts), one joins two rows.  The owned rows of the state and the links' records -- a link's record is the
one of the strip that owns its end a, as StripRunner.gather_links takes it -- are compared with the single domain's after every batch.
usage: links_strips_worker.py <world> <reaches: 1 | 2>"""
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
import test_links as T  # noqa: E402

world, reaches = int(sys.argv[1]), int(sys.argv[2])
batches = [8, 12, 20]                                  # 40 iterations in even batches
g = strips.ghost_rows(hp.SCHEME_GODUNOV) * reaches
st, bed, man, links = T.scene()
links = links + [dict(a=(18, 15), b=(21, 15), kind=T.WEIR, level=1.5, size=1.0, coeff=1.7, limit=0.6),       # next to the cut of two strips
                 dict(a=(21, 16), b=(18, 16), kind=T.ORIFICE, level=0.5, size=0.5, coeff=0.6, limit=np.inf),
                 dict(a=(18, 9), b=(21, 9), kind=T.ORIFICE, level=0.5, size=0.5, coeff=0.6, limit=np.inf),    # ... and of three
                 dict(a=(18, 21), b=(21, 21), kind=T.WEIR, level=1.5, size=1.0, coeff=1.7, limit=0.6),
                 dict(a=(10, 5), b=(30, 7), kind=T.ORIFICE, level=0.0, size=0.5, coeff=0.6, limit=np.inf)]    # across rows, inside one strip
packed = hp.pack_links(links, T.COLS)
parts = strips.partition(T.ROWS, world, g)
assert strips.links_refused(packed, T.COLS, parts, strips.ghost_rows(hp.SCHEME_GODUNOV)) is None
rows_a = (packed["cell_a"] // np.uint64(T.COLS)).astype(np.int64)
rows_b = (packed["cell_b"] // np.uint64(T.COLS)).astype(np.int64)
stored_by = [sum(1 for _, _, lo, hi in parts if lo <= ra < hi and lo <= rb < hi) for ra, rb in zip(rows_a, rows_b)]


def prepare(dom):
    dom.set_target_time(1e9)
    dom.add_uniform(T.RAIN["definition"], T.RAIN["series"], T.RAIN["interval"], T.RAIN["length"])
    dom.add_links(packed)


single = hp.Domain(T.COLS, T.ROWS, dx=T.DX)
single.upload(st, bed, man)
prepare(single)
single.update_timestep()
want = []
for n in batches:
    single.step_batch(n)
    want.append((single.download(), single.links_read()))
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
        dom = hp.Domain(T.COLS, hi - lo, dx=T.DX, global_rows=T.ROWS, row_offset=lo, ghost_rows=g if reaches > 1 else 0)
        dom.upload(st[lo:hi], bed[lo:hi], man[lo:hi])
        dom.strip_comm_init(uid, r, world)
        tickets[r] = dom.strip_peer_ticket()
        start.wait()
        dom.strip_peer_connect(tickets, r)
        start.wait()
        prepare(dom)
        dom.strip_update_timestep()
        mine = np.flatnonzero((rows_a >= own_lo) & (rows_a < own_hi))
        for k, n in enumerate(batches):
            dom.strip_step_batch(n)
            local = dom.download()
            got[k][r] = (local[own_lo - lo:own_hi - lo].copy(), mine, dom.links_read()[mine])
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
same_state, same_records = [], []
for k in range(len(batches)):
    state = np.concatenate([p[0] for p in got[k]], axis=0)
    rec = np.zeros(len(packed), hp.LINK_RECORD_DTYPE)
    for _, idx, r in got[k]:
        rec[idx] = r
    same_state.append(bool(np.array_equal(state, want[k][0])))
    same_records.append(bool(rec.tobytes() == want[k][1].tobytes()))
moved = int((want[-1][1]["active"] > 0).sum())
ok = all(same_state) and all(same_records) and moved >= 8 and max(stored_by) == 2 and min(stored_by) == 1
print("world", world, "reaches", reaches, "state identical", same_state, "records identical", same_records, "links that moved", moved, "stored by", stored_by, flush=True)
print("the strips are the single domain True" if ok else "FAILED", flush=True)
os._exit(0 if ok else 1)
