"""Launched by torch.distributed.run from tests/test_gpu_output_stage.py: one rank of a strip-decomposed run with the HIP
engine, several process ranks sharing GPU 0, exchange staged through host memory over gloo (the rehearsal transport of
strip_rehearsal_worker.py).  After the run every rank calls StripRunner.gather_outputs (fp64 and fp32) and
StripRunner.gather_stats; rank 0 saves what they returned, every rank reports whether gather_outputs gave it rasters."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "hipims-ocl_amd"))

from hipims_mi import strips, synthetic as syn  # noqa: E402

NAMES = ["depth", "maxdepth", "fsl", "maxfsl", "dischargex", "dischargey", "velocityx", "velocityy", "froude"]


def main():
    out, scheme, cols, rows, steps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    st, bed, man = syn.s_rough(cols, rows, manning=None)
    r = strips.StripRunner(cols, rows, scheme=scheme, rank=rank, world=world, device=0, backend="gloo")
    r.upload_global(st, bed, man)
    r.set_target_time(1e9)
    r.step(steps)
    r.barrier()
    rasters = r.gather_outputs(NAMES)
    rasters32 = r.gather_outputs(["depth", "froude"], dtype=np.float32)
    stats = r.gather_stats()
    got = [None] * world
    r.dist.all_gather_object(got, (rasters is not None, stats))
    if rank == 0:
        assert [g[0] for g in got] == [True] + [False] * (world - 1), got      # rank 0 alone receives the rasters
        assert all(g[1] == stats for g in got), got                             # every rank has the same statistics
        np.savez(out, **{"f64_" + n: rasters[n] for n in NAMES}, **{"f32_" + n: a for n, a in rasters32.items()},
                 **{"stats_" + k: (-1 if v is None else v) for k, v in stats.items()})
    r.close()


if __name__ == "__main__":
    main()
