"""A traced run against an untraced one held to single iterations (HP_TWO_STEP=0, set here before the library loads: the switch is
read once per process): the scene of tests/test_links.py with the rain and the cell inflow, 24 iterations in batches of 1, 3 and
7, state and scalars compared after every batch.  usage: python tracer_untraced_worker.py fast|strict f64|f32"""
import os
import sys

os.environ["HP_TWO_STEP"] = "0"
os.environ["HIPIMS_MI_NO_TORCH"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "hipims-ocl_amd")]

import numpy as np

import hipims_mi as hp
import test_links as T
import test_tracer as TT


def main():
    math_mode = hp.MATH_STRICT if sys.argv[1] == "strict" else hp.MATH_FAST
    precision = sys.argv[2]
    st, bed, man, _ = T.scene(np.float64 if precision == "f64" else np.float32)
    doms = []
    for traced in (True, False):
        dom = hp.Domain(T.COLS, T.ROWS, dx=T.DX, precision=precision, math_mode=math_mode)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        dom.add_uniform(T.RAIN["definition"], T.RAIN["series"], T.RAIN["interval"], T.RAIN["length"])
        dom.add_cell(T.INFLOW["depth_def"], T.INFLOW["discharge_def"], T.INFLOW["cells"], T.INFLOW["series"], T.INFLOW["interval"], T.INFLOW["length"])
        if traced:
            dom.tracer_enable(TT.blob())
            dom.tracer_add_source(TT.SOURCE["cells"], TT.SOURCE["series"])
        doms.append(dom)
    a, b = doms
    same = True
    device = lambda sc: {k: v for k, v in sc.items() if k not in ("cells_calculated", "iterations")}
    for k, n in enumerate([1, 3, 7, 1, 3, 7, 2]):
        a.step_batch(n)
        b.step_batch(n)
        ok = np.array_equal(a.download(), b.download()) and device(a.read_scalars()) == device(b.read_scalars())
        print("batch", k, "equal", ok, flush=True)
        same = same and ok
    moved = not np.array_equal(a.tracer_read(), TT.blob())
    print("pairs", a.pair_stats()["pairs"], b.pair_stats()["pairs"], "tracer iterations", a.tracer_info()["iterations"], "moved", moved)
    verdict = same and moved and a.pair_stats()["pairs"] == 0 and b.pair_stats()["pairs"] == 0 and a.tracer_info()["iterations"] == 24
    print("the traced run is the untraced run", verdict)
    a.close(); b.close()
    return 0 if verdict else 1


if __name__ == "__main__":
    sys.exit(main())
