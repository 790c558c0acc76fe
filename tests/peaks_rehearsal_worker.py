"""Launched by torch.distributed.run from tests/test_gpu_peaks.py: one rank of a strip-decomposed run with the HIP engine,
process ranks sharing GPU 0, exchange staged through host memory over gloo (the rehearsal transport of
strip_rehearsal_worker.py).  Every rank calls StripRunner.peaks_enable, takes a StripRunner.peaks_sample after every batch and
then StripRunner.gather_peaks (fp64 and fp32); rank 0 saves what they returned and checks that it alone received rasters.
usage: peaks_rehearsal_worker.py <out.npz> <cols> <rows> <batch> [<batch> ...]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "hipims-ocl_amd"))

import hipims_mi as hp  # noqa: E402
from hipims_mi import strips, synthetic as syn  # noqa: E402

NAMES = list(hp.PEAK_CODES)


def main():
    out, cols, rows, batches = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), [int(a) for a in sys.argv[4:]]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    st, bed, man = syn.s_rough(cols, rows, manning=None)
    r = strips.StripRunner(cols, rows, rank=rank, world=world, device=0, backend="gloo")
    r.upload_global(st, bed, man)
    r.set_target_time(1e9)
    r.peaks_enable(NAMES, arrival_depth=0.02)
    for n in batches:
        r.step(n)
        r.peaks_sample()
    r.barrier()
    rasters = r.gather_peaks(NAMES)
    rasters32 = r.gather_peaks(["hazard", "wetduration"], dtype=np.float32)
    info = r.engine.peaks_info()
    got = [None] * world
    r.dist.all_gather_object(got, (rasters is not None, rasters32 is not None, info))
    if rank == 0:
        assert [g[:2] for g in got] == [(True, True)] + [(False, False)] * (world - 1), got      # rank 0 alone receives the rasters
        assert all(g[2] == info for g in got), got                                                # every rank took the same samples
        np.savez(out, info=np.array([info["samples"], info["t_first"], info["t_last"]]),
                 **{"f64_" + n: rasters[n] for n in NAMES}, **{"f32_" + n: a for n, a in rasters32.items()})
    r.close()


if __name__ == "__main__":
    main()
