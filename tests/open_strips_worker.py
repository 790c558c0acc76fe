"""Worker of tests/test_gpu_open.py::test_strips: WORLD strips as threads of this process on the one GPU (the library's own strip loop
over tests/fake_rccl, as links_strips_worker.py), one reach of ghost rows.  Every rank adds the rain and then every segment with GLOBAL
indices, which is what StripRunner.add_open does on each rank.  The owned rows of the state and the records -- a cell's record is the one
of the strip that owns its row, as StripRunner.gather_open takes it -- are compared with the single domain's after every batch.  A strip
with two reaches of ghost rows is refused.
usage: open_strips_worker.py <world>"""
import ctypes as C
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd"), os.path.join(ROOT, "tests")]
os.environ["HIPIMS_MI_NO_TORCH"] = "1"
os.environ["GPU_MAX_HW_QUEUES"] = "24"          # every rank's streams on hardware queues of their own (strip_threads_worker.py)
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
from hipims_mi import frontend, strips  # noqa: E402
import oracle  # noqa: E402
import test_links as T  # noqa: E402
import test_open as O  # noqa: E402

world = int(sys.argv[1])
batches = [8, 12, 20, 20]                              # 60 iterations
g = strips.ghost_rows(hp.SCHEME_GODUNOV)
st, bed, man = O.scene()
segments = O.SEGMENTS + [dict(edge="west", first=12, last=20)]        # west and east cells on both sides of a cut, and on ghost rows
packed = hp.pack_open_segments(segments, T.COLS, T.ROWS)
for c in range(12, 21):                                               # the west ring opened like the others: a real bed below its neighbour's
    bed[c, 0] = bed[c, 1] - 0.02
    st[c, 0, :2] = bed[c, 0]
parts = strips.partition(T.ROWS, world, g)
layout = frontend.Open(T.ROWS, T.COLS, T.DX, oracle.OracleFunctions("f64", dx=T.DX), segments)
rows = layout.ry.astype(np.int64)


def prepare(dom):
    dom.set_target_time(1e9)
    dom.add_uniform(T.RAIN["definition"], T.RAIN["series"], T.RAIN["interval"], T.RAIN["length"])
    dom.add_open(packed)


single = hp.Domain(T.COLS, T.ROWS, dx=T.DX)
single.upload(st, bed, man)
prepare(single)
single.update_timestep()
want = []
for n in batches:
    single.step_batch(n)
    want.append((single.download(), single.open_read()))
single.close()

# a strip with two reaches of ghost rows is refused, and stays without an open boundary
lo, hi = strips.partition(T.ROWS, 2, 2 * g)[0][2:]
two = hp.Domain(T.COLS, hi - lo, dx=T.DX, global_rows=T.ROWS, row_offset=lo, ghost_rows=2 * g)
two.upload(st[lo:hi], bed[lo:hi], man[lo:hi])
refused = two.lib.hp_boundary_add_open(two.h, packed.ctypes.data_as(C.c_void_p), len(packed)) == -4 and two.open_info() == dict(segments=0, cells=0)
two.close()

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
        prepare(dom)
        dom.strip_update_timestep()
        mine = np.flatnonzero((rows >= own_lo) & (rows < own_hi))
        for k, n in enumerate(batches):
            dom.strip_step_batch(n)
            local = dom.download()
            got[k][r] = (local[own_lo - lo:own_hi - lo].copy(), mine, dom.open_read()[mine])
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
    rec = np.zeros(len(rows), hp.OPEN_RECORD_DTYPE)
    for _, idx, r in got[k]:
        rec[idx] = r
    same_state.append(bool(np.array_equal(state, want[k][0])))
    same_records.append(bool(rec.tobytes() == want[k][1].tobytes()))
left = int((want[-1][1]["active"] > 0).sum())
ok = all(same_state) and all(same_records) and left >= 10 and refused
print("world", world, "state identical", same_state, "records identical", same_records, "cells water left through", left, "two reaches refused", refused, flush=True)
print("the strips are the single domain True" if ok else "FAILED", flush=True)
os._exit(0 if ok else 1)
