"""Worker of tests/test_gpu_links.py::test_no_pairs_with_links: run with HP_TWO_STEP=1 (read once by the library), a domain with a
link group runs single iterations only (hp_pair_stats' first word stays 0) and runs iteration pairs again once hp_boundary_clear has
removed the group."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
import test_links as T  # noqa: E402

assert os.environ.get("HP_TWO_STEP") == "1"
st, bed, man, links = T.scene()
# FAST arithmetic: in STRICT the engine chooses between pairs and single iterations by measurement, so pairs after the clear are not owed
dom = hp.Domain(T.COLS, T.ROWS, dx=T.DX, math_mode=hp.MATH_FAST)
dom.upload(st, bed, man)
dom.set_target_time(1e9)
dom.add_links(links)
fused = dom.boundaries_fused()
dom.step_batch(20)
with_links = dom.pair_stats()["pairs"]
moved = int(dom.links_read()["active"].sum())
dom.clear_boundaries()
info = dom.links_info()
dom.step_batch(20)
without = dom.pair_stats()["pairs"]
finite = bool(np.isfinite(dom.download()).all())
print("fused", fused, "pairs with links", with_links, "links moved", moved, "after clear", info, "pairs", without, "finite", finite, flush=True)
ok = not fused and with_links == 0 and moved > 0 and info == dict(links=0, groups=0) and without > 0 and finite
dom.close()
print("no pairs with links, pairs without" if ok else "FAILED", flush=True)
sys.exit(0 if ok else 1)
