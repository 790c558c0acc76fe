"""Worker of tests/test_gpu_links.py::test_a_domain_with_links_never_speculates (HP_STRICT_SPECULATE / HP_STRICT_SPEC_FORCE are read
once per process; the caller sets both to 1, so that every speculative batch is run again): a STRICT fp64 domain with the scene's
links, three batches of 9 iterations, against the stepwise reference loop.  A batch that was queued twice would count the links'
records twice.  A domain without links, in the same process, shows that batches of this size do speculate here."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
from hipims_mi import frontend  # noqa: E402
import test_links as T  # noqa: E402

assert os.environ.get("HP_STRICT_SPECULATE") == "1" and os.environ.get("HP_STRICT_SPEC_FORCE") == "1"
logs = []
hp.set_log_sink(lambda level, text: logs.append(text))
replays = lambda: sum("re-run with the plain divisions" in l for l in logs)
st, bed, man, links = T.scene()


def domain():
    dom = hp.Domain(T.COLS, T.ROWS, dx=T.DX, math_mode=hp.MATH_STRICT)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    return dom


plain = domain()
for _ in range(3):
    plain.step_batch(9)
    plain.sync()
plain.read_scalars()
without = replays()
plain.close()

dom = domain()
dom.add_links(links)
L = frontend.Links(T.ROWS, T.COLS, T.DX, links)
loop = T.StepLoop(st, bed, man, [("links", L)])
same = []
for _ in range(3):
    dom.step_batch(9)
    loop.step(9)
    same.append(bool(np.array_equal(dom.download(), loop.download()) and dom.links_read().tobytes() == L.records().tobytes()))
with_links = replays() - without
moved = int(L.records()["active"].sum())
dom.close()
ok = without == 3 and with_links == 0 and all(same) and moved > 20
print("replays without links", without, "with links", with_links, "state and records are the reference's", same, "links moved", moved, flush=True)
print("a domain with links never speculates" if ok else "FAILED", flush=True)
sys.exit(0 if ok else 1)
