"""Worker of tests/test_gpu_peaks.py::test_samples_behind_speculative_strict_batches (HP_STRICT_SPECULATE / HP_STRICT_SPEC_FORCE
are read once per process): three STRICT fp64 batches of 9 iterations, a sample after each, the peaks saved to <out>.
usage: peaks_spec_worker.py <out.npz>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
import hipims_mi as hp  # noqa: E402
from hipims_mi import synthetic as syn  # noqa: E402

logs = []
hp.set_log_sink(lambda level, text: logs.append(text))
cols, rows = 190, 101
st, bed, man = syn.s_rough(cols, rows, manning=None, seed=31)
dom = hp.Domain(cols, rows, math_mode=hp.MATH_STRICT)
dom.upload(st, bed, man)
dom.set_target_time(1e9)
dom.peaks_enable(list(hp.PEAK_CODES))
for _ in range(3):
    dom.step_batch(9)
    dom.peaks_sample()                  # enters the library behind a batch that may still have to be re-run
peaks, info, state = dom.peaks(), dom.peaks_info(), dom.download()
dom.close()
np.savez(sys.argv[1], state=state, info=np.array([info["samples"], info["t_first"], info["t_last"]]), **peaks)
print("replays=%d" % sum("re-run with the plain divisions" in l for l in logs))
