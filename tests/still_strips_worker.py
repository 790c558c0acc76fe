"""Worker of tests/test_gpu_still_pairs.py: row strips (three ranks as threads of this process on the one GPU, over the test double of
the collective library, two reaches of ghost rows so that the strips run iteration pairs with TAIL 2 -- the ghost rows of the
neighbours written through store_peer, still runs included) on a dam break beside still water, against the single domain, bit
for bit.  Prints "bit-identical True" on success.   usage: still_strips_worker.py"""
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
os.environ["HIPIMS_MI_NO_TORCH"] = "1"
os.environ["GPU_MAX_HW_QUEUES"] = "24"             # (as tests/strip_threads_worker.py: the ranks' streams on queues of their own)
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
from hipims_mi import strips, synthetic as syn  # noqa: E402

world, period = 3, 2
cols, rows = 1030, 900
st, bed, man = syn.s_dam(cols, rows)
st[:, :, 2:] = 0.0
st[300:600, 700:1000, 1] = st[300:600, 700:1000, 0] - 0.5          # Zmax below Z in the still pool
bed[450, 520:1029] = 6.0
st[450, 520:1029, 0] = 6.0
st[450, 520:1029, 1] = 6.0
g = strips.ghost_rows(hp.SCHEME_GODUNOV) * period
parts = strips.partition(rows, world, g)
batches = [40, 7, 64, 31]

single = hp.Domain(cols, rows)
single.upload(st, bed, man); single.set_target_time(1e9)
single.update_timestep()
single.step_batch(sum(batches))
want, want_sc = single.download(), single.read_scalars()
single.close()

lib = hp.load_library()
hp._check(lib, lib.hp_comm_load(os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so").encode()), "hp_comm_load")
uid = hp.comm_unique_id()
got, scal, launches, errors = [None] * world, [None] * world, [None] * world, []
start = threading.Barrier(world)
tickets = [None] * world


def rank_main(r):
    try:
        own_lo, own_hi, lo, hi = parts[r]
        dom = hp.Domain(cols, hi - lo, global_rows=rows, row_offset=lo, ghost_rows=g)
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
        dom.sync()
        got[r] = dom.download()[own_lo - lo:own_hi - lo]
        scal[r] = dom.read_scalars()
        launches[r] = dom.launch_counts()[0]
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
out = np.concatenate(got, axis=0)
same = np.array_equal(out.view(np.uint64), want.view(np.uint64))
if not same:
    bad = np.argwhere(out.view(np.uint64) != want.view(np.uint64))
    print("differing words", len(bad), "first", bad[:6].tolist(), "strip edges", [pp[:2] for pp in parts], flush=True)
times = {(s["time"], s["timestep"]) for s in scal}
print("flux launches per rank", launches, "iterations", sum(batches), "bit-identical", same, "times", times,
      "single", (want_sc["time"], want_sc["timestep"]), flush=True)
paired = all(n < 0.62 * sum(batches) for n in launches)                   # the strips ran iteration pairs
print("pairs taken", paired, flush=True)
os._exit(0 if same and paired and times == {(want_sc["time"], want_sc["timestep"])} else 1)
