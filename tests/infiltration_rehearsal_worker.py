"""Launched by torch.distributed.run from tests/test_gpu_infiltration.py: one rank of a strip-decomposed run with the HIP engine,
process ranks sharing GPU 0, exchange staged through host memory over gloo after every iteration (the rehearsal transport of
strip_rehearsal_worker.py).  Every rank calls StripRunner.add_infiltration with the WHOLE grid's soil raster and a hot start that
differs from cell to cell, runs the batches and calls StripRunner.gather_infiltration; rank 0 saves what it returned, with the
gathered state, and checks that it alone received a raster.
usage: infiltration_rehearsal_worker.py <out.npz> <batch> [<batch> ...]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd"), HERE]

from hipims_mi import strips  # noqa: E402
import test_infiltration as TI  # noqa: E402
import test_links as T  # noqa: E402


def main():
    out, batches = sys.argv[1], [int(a) for a in sys.argv[2:]]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    st, bed, man, soil = TI.soil_scene()
    r = strips.StripRunner(T.COLS, T.ROWS, rank=rank, world=world, device=0, backend="gloo", dx=T.DX)
    assert r.exchange_period == 1
    r.upload_global(st, bed, man)
    r.set_target_time(1e9)
    r.domain.add_uniform(T.RAIN["definition"], T.RAIN["series"], T.RAIN["interval"], T.RAIN["length"])
    r.add_infiltration(soil, TI.CLASSES, TI.hot_start_raster())
    for n in batches:
        r.step(n)
    r.barrier()
    state = r.gather_owned()
    F = r.gather_infiltration()
    got = [None] * world
    r.dist.all_gather_object(got, F is not None)
    if rank == 0:
        assert got == [True] + [False] * (world - 1), got
        np.savez(out, state=state, F=F)
    r.close()


if __name__ == "__main__":
    main()
