"""Block order of the FAST fp64 pair kernel's record launches (hp_order.hpp; hp_kernels.hpp: OrderHook; round 18): the column groups
whose waves marched in one launch get their tiles dealt first in the next.  Which block runs which tile must change no bit and no launch
count, so every case holds the default run to the same run in tile-row order (HP_PAIR_ORDER=0) and to single iterations (HP_TWO_STEP=0)
-- as bit patterns.  hp_pair_stats out[11] says whether a launch really ran out of tile-row order: it must where one column group
marches among still ones, and must not where none or every one does.

The grids (tests/pair_order_worker.py): 722 x 130, three column groups, and 482 x 75, two groups and bands that are no multiple of the
8-row tiles.  S-DAM itself (`dam`) has a closed edge ring, whose columns never match the pool beside them: the first and the last column
group march in every launch, with the dam's in the middle that is every group of either grid -- so `dam` runs on a third grid as well,
1262 x 75 with six groups, where three groups stand still between them and the launches must be seen reordered; `dam_open`, the same
pools with the ring at their level, is the scene in which only the middle group of the three marches."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
WORKER = os.path.join(HERE, "pair_order_worker.py")
GRIDS = ("722x130", "482x75")


def run(case, tmp_path, order, two_step=1, skip=1):
    out = os.path.join(str(tmp_path), f"{case}_{order}_{two_step}_{skip}.npz")
    r = subprocess.run([sys.executable, WORKER, case, out], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, HP_PAIR_ORDER=str(order), HP_TWO_STEP=str(two_step), HP_PAIR_SKIP=str(skip), HP_MARCH2_RSEG="8"))
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout, end="")
    return np.load(out)


def grids(a):
    return [k[:-len("_state")] for k in a.files if k.endswith("_state")]


def same_bits(a, b, what, launches=True):
    assert grids(a) == grids(b)
    for g in grids(a):
        ca, cb = a[g + "_counts"], b[g + "_counts"]
        assert int(ca[0]) == int(cb[0]), f"{what} {g}: iterations {ca[0]} / {cb[0]}"
        if launches:
            assert ca.tolist() == cb.tolist(), f"{what} {g}: launch counts {ca.tolist()} / {cb.tolist()}"
        assert a[g + "_scalars"].view(np.uint64).tolist() == b[g + "_scalars"].view(np.uint64).tolist(), f"{what} {g}: t, dt"
        x, y = a[g + "_state"].view(np.uint64), b[g + "_state"].view(np.uint64)
        assert x.shape == y.shape
        bad = np.argwhere(x != y)
        assert bad.size == 0, f"{what} {g}: {len(bad)} words differ, first at {bad[:5].tolist()}"


def check(case, tmp_path, skip=1):
    on, off = run(case, tmp_path, 1, skip=skip), run(case, tmp_path, 0, skip=skip)
    for g in grids(on):
        assert int(on[g + "_counts"][1]) < int(on[g + "_counts"][0]) * 0.8      # pairs were taken
        assert int(off[g + "_moved"].max()) == 0                               # HP_PAIR_ORDER=0: tile-row order throughout
    same_bits(on, off, "HP_PAIR_ORDER=0")
    same_bits(on, run(case, tmp_path, 1, two_step=0, skip=skip), "single iterations", launches=False)
    return on


def test_dam(tmp_path):
    on = check("dam", tmp_path)
    assert int(on["722x130_skipped"].max()) > 0              # (482 x 75: every window lies beside the ring, the dam or such a window)
    # the benchmark's own scene, reordered: on the six-group grid the groups between the dam's and the ring's stand still
    assert int(on["1262x75_moved"].max()) > 0, on["1262x75_moved"].tolist()
    assert int(on["1262x75_skipped"].max()) > 0


def test_dam_open_runs_the_middle_group_first(tmp_path):
    on = check("dam_open", tmp_path)
    assert int(on["722x130_moved"].max()) > 0, on["722x130_moved"].tolist()
    assert int(on["482x75_moved"].max()) == 0                # the dam lies on the border of its two groups: both march
    assert int(on["722x130_skipped"].max()) > 0


def test_front_in_the_last_group_only(tmp_path):
    on = check("edge_front", tmp_path)
    for g in GRIDS:
        assert int(on[g + "_moved"].max()) > 0, (g, on[g + "_moved"].tolist())


def test_still_water_keeps_tile_row_order_and_is_skipped(tmp_path):
    on = check("still", tmp_path)
    for g in GRIDS:
        assert int(on[g + "_moved"].max()) == 0, (g, on[g + "_moved"].tolist())
        assert int(on[g + "_skipped"].max()) > 0


def test_rough_flags_every_group(tmp_path):
    on = check("rough", tmp_path)
    for g in GRIDS:
        assert int(on[g + "_moved"].max()) == 0, (g, on[g + "_moved"].tolist())


def test_interleaved_batches_checkpoint_and_upload(tmp_path):
    on = check("interleave", tmp_path)
    assert int(on["722x130_moved"].max()) > 0


def test_fixed_timestep(tmp_path):
    on = check("fixed", tmp_path)
    assert int(on["722x130_moved"].max()) > 0


def test_flags_and_order_without_records(tmp_path):
    on = check("dam_open", tmp_path, skip=0)
    assert int(on["722x130_moved"].max()) > 0
    for g in GRIDS:
        assert int(on[g + "_skipped"].max()) == 0
