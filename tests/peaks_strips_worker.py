"""Worker of tests/test_gpu_peaks.py::test_strips_gather_peaks: WORLD strips as threads of this process on the one GPU (the
library's own strip loop over tests/fake_rccl, as output_strips_worker.py).  Every rank tracks its own strip -- a sample after
every batch, nothing exchanged -- and reads the rows it OWNS, which is what StripRunner.peaks_enable / peaks_sample / gather_peaks
do on each rank; the parts are put together by the function gather_peaks uses (strips.assemble_outputs; the transport between
the ranks, torch.distributed there, is a list here) and compared with the single domain's peaks.
usage: peaks_strips_worker.py <world>"""
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
NAMES = list(hp.PEAK_CODES)
cols, rows, batches = 96, 70, [3, 4, 5, 2, 1, 8]
g = strips.ghost_rows(hp.SCHEME_GODUNOV)
st, bed, man = syn.s_rough(cols, rows)
parts = strips.partition(rows, world, g)

single = hp.Domain(cols, rows)
single.upload(st, bed, man); single.set_target_time(1e9)
single.update_timestep()
single.peaks_enable(NAMES)
for n in batches:
    single.step_batch(n)
    single.peaks_sample()
want, want32, want_info = single.peaks(), single.peaks(dtype=np.float32), single.peaks_info()
single.close()

lib = hp.load_library()
hp._check(lib, lib.hp_comm_load(os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so").encode()), "hp_comm_load")
uid = hp.comm_unique_id()
rasters, rasters32, infos, errors = [None] * world, [None] * world, [None] * world, []
tickets = [None] * world
start = threading.Barrier(world)


def rank_main(r):
    try:
        own_lo, own_hi, lo, hi = parts[r]
        dom = hp.Domain(cols, hi - lo, global_rows=rows, row_offset=lo)
        dom.upload(st[lo:hi], bed[lo:hi], man[lo:hi])
        dom.strip_comm_init(uid, r, world)
        dom.set_target_time(1e9)
        tickets[r] = dom.strip_peer_ticket()
        start.wait()
        dom.strip_peer_connect(tickets, r)
        start.wait()
        dom.strip_update_timestep()
        dom.peaks_enable(NAMES)
        for n in batches:
            dom.strip_step_batch(n)
            dom.peaks_sample()
        rasters[r] = dom.peaks(NAMES, row0=own_lo - lo, nrows=own_hi - own_lo)
        rasters32[r] = dom.peaks(NAMES, dtype=np.float32, row0=own_lo - lo, nrows=own_hi - own_lo)
        infos[r] = dom.peaks_info()
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
tracked = all((want[n] != -9999.0).any() for n in NAMES)
print("ranks", world, "peaks bit-identical", same, "every value tracked somewhere", tracked, "info equal", all(i == want_info for i in infos), flush=True)
os._exit(0 if same and tracked and all(i == want_info for i in infos) else 1)
