"""Worker of tests/test_gpu_output_stage.py::test_strips_gather_outputs_and_stats: WORLD strips as threads of this process on
the one GPU (the library's own strip loop over tests/fake_rccl, as strip_threads_worker.py).  After the batches every rank
derives the rasters and the statistics of the rows it OWNS on its device -- what StripRunner.gather_outputs / gather_stats do
on each rank --; the parts are put together by the functions those two use (strips.assemble_outputs, strips.combine_stats;
the transport between the ranks, torch.distributed there, is a list here) and compared with the single domain's.
usage: output_strips_worker.py <world> <scheme 0|1>"""
import math
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

world, scheme = int(sys.argv[1]), int(sys.argv[2])
NAMES = ["depth", "maxdepth", "fsl", "maxfsl", "dischargex", "dischargey", "velocityx", "velocityy", "froude"]
cols, rows, batches = 300, 157, [1, 2, 57]
g = strips.ghost_rows(scheme)                   # 1 (Godunov) or 2 (MUSCL-Hancock) ghost rows per interior side
st, bed, man = syn.s_rough(cols, rows)
parts = strips.partition(rows, world, g)

single = hp.Domain(cols, rows, scheme=scheme)
single.upload(st, bed, man); single.set_target_time(1e9)
single.update_timestep()
single.step_batch(sum(batches))
want, want_stats, want_state = single.derive(NAMES), single.stats(), single.download()
want32 = single.derive(NAMES, dtype=np.float32)
single.close()

lib = hp.load_library()
hp._check(lib, lib.hp_comm_load(os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so").encode()), "hp_comm_load")
uid = hp.comm_unique_id()
rasters, rasters32, stats, errors = [None] * world, [None] * world, [None] * world, []
tickets = [None] * world
start = threading.Barrier(world)


def rank_main(r):
    try:
        own_lo, own_hi, lo, hi = parts[r]
        dom = hp.Domain(cols, hi - lo, scheme=scheme, global_rows=rows, row_offset=lo)
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
        rasters[r] = dom.derive(NAMES, row0=own_lo - lo, nrows=own_hi - own_lo)
        rasters32[r] = dom.derive(NAMES, dtype=np.float32, row0=own_lo - lo, nrows=own_hi - own_lo)
        stats[r] = dom.stats(row0=own_lo - lo, nrows=own_hi - own_lo)
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
got, got32 = strips.assemble_outputs(rasters), strips.assemble_outputs(rasters32)
same = all(np.array_equal(got[n], want[n]) and np.array_equal(got32[n], want32[n]) for n in NAMES)
total = strips.combine_stats(stats, [p[2] for p in parts], cols)
exact = all(total[k] == want_stats[k] for k in ("cells", "cells_wet", "max_depth", "max_speed", "max_depth_cell", "max_speed_cell"))
# the volume: against the correctly rounded sum of the same terms; (n - 1) 2^-53 bounds ANY order of adding n non-negative terms
z, zmax, zb = want_state[..., 0], want_state[..., 1], bed
counted = (zmax > -9999.0) & (zb <= 9999.0)
ref = math.fsum(np.maximum(0.0, z - zb)[counted])
err = abs(total["volume"] - ref) / ref
bound = (int(counted.sum()) - 1) * 2.0 ** -53
print("ranks", world, "scheme", scheme, "volume", total["volume"], "fsum", ref, "relative error %.3e bound %.3e" % (err, bound),
      "wet cells", total["cells_wet"], "rasters bit-identical", same, "statistics equal", exact and err <= bound and int(counted.sum()) == total["cells"], flush=True)
os._exit(0 if same and exact and err <= bound else 1)
