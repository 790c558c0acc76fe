"""Launched by torch.distributed.run from tests/test_gpu_zones.py: one rank of a strip-decomposed run with the HIP engine,
process ranks sharing GPU 0, exchange staged through host memory over gloo (the rehearsal transport of
strip_rehearsal_worker.py).  Every rank calls StripRunner.zones_enable with the WHOLE grid's raster, takes a
StripRunner.zones_sample after every batch and then StripRunner.gather_zones; rank 0 saves what it returned and checks that it
alone received a series.  The device buffer holds 4 records: it is drained along the way.
usage: zones_rehearsal_worker.py <out.npz> <ids.npy> <zone_count> <flood_depth> <dx> <batch> [<batch> ...]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "hipims-ocl_amd"))

from hipims_mi import strips, synthetic as syn  # noqa: E402


def main():
    out, ids, zone_count, flood, dx = sys.argv[1], np.load(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), float(sys.argv[5])
    batches = [int(a) for a in sys.argv[6:]]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    rows, cols = ids.shape
    st, bed, man = syn.s_rough(cols, rows)
    r = strips.StripRunner(cols, rows, rank=rank, world=world, device=0, backend="gloo", dx=dx)
    r.upload_global(st, bed, man)
    r.set_target_time(1e9)
    r.zones_enable(ids, zone_count, flood_depth=flood, capacity=4)
    assert r._zone_host is None                            # the HIP engine records on the device
    for n in batches:
        r.step(n)
        r.zones_sample()
    r.barrier()
    series = r.gather_zones()
    info = r.engine.zones_info()
    got = [None] * world
    r.dist.all_gather_object(got, (series is not None, info["samples"], info["stride"]))
    if rank == 0:
        assert got == [(True, len(batches), 1 + 7 * zone_count)] + [(False, len(batches), 1 + 7 * zone_count)] * (world - 1), got
        np.savez(out, **series)
    r.close()


if __name__ == "__main__":
    main()
