"""Still water beside the edge ring in the FAST fp64 pair kernel (hp_kernels.hpp: godunov_march2, wall_ok; round 19): a window next to
the ring takes its lake in still runs, and its tiles are skipped, once the wave has checked with the march's own update that this lake
stays as it is beside this wall.  That must change no bit, so every case holds the default run to the run without that part
(HP_PAIR_WALL=0) and, where stated, to the run without any records (HP_PAIR_SKIP=0) -- as bit patterns, so that a -0.0 counts.  Every
setting is a fresh child process (the switches are read once per process).

The precondition.  A comparison of two full marches proves nothing, so every case first asserts that its reference, HP_PAIR_WALL=0,
skipped interior tiles.  Without the wall part a tile is skipped only if the windows either side of it wrote records, which a window
beside the ring never does: the reference can skip from five windows across on (302 columns: the middle one), and every case that can
runs there.  At 122 columns (two windows, both beside the ring) and 242 (four: the two inner ones each have a ring window for a
neighbour) the reference cannot skip whatever the code does; those shapes are here for their geometry, and their cases
assert instead that the reference took pairs and that the DEFAULT run skipped -- a comparison of skipped tiles with a full march.

The pair whose wall term survives.  hp_math.hpp (face_solve_fast) keeps the half ulp of the wall's bed that the reference's shifted
levels carry; times g/2 h it passes the update's flush of 1e-10 where h is large enough, and the lake then starts to move at its
walls.  Searched on the CPU with the oracle (a 14 x 10 box of one level inside the 9999.9 wall, four iterations): levels 10, 1, 50, 100,
500.5 and 1000 over a bed of 0, 2.5 over 0.5 and 12.3456 over 1.1 stay at rest in every bit; 75.3 over 0, 30.3 over 0.1 and 200.7 over
3.3 move in the cells along the walls (a level the subtraction from 9999.9 does not return exactly).  SURVIVING is the first of these."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
WORKER = os.path.join(HERE, "wall_still_worker.py")
_runs = {}

# (level, bed, wall bed) of a still lake that moves at its walls in the oracle -- found there before it was fixed here
SURVIVING = (75.3, 0.0, 9999.9)


def run(tmp_path_factory, case, cols, rows, wall=1, skip=1, rseg=None, lake=()):
    """One worker run, shared among the tests that need it (nothing changes a result once it is loaded)."""
    key = (case, cols, rows, wall, skip, rseg, lake)
    if key not in _runs:
        out = os.path.join(str(tmp_path_factory.mktemp("wall")), "out.npz")
        env = dict(os.environ, HP_TWO_STEP="1", HP_PAIR_EXACT="0", HP_PAIR_WALL=str(wall), HP_PAIR_SKIP=str(skip))
        env.pop("HP_MARCH2_RSEG", None)
        if rseg is not None:
            env["HP_MARCH2_RSEG"] = str(rseg)
        r = subprocess.run([sys.executable, WORKER, case, str(cols), str(rows), out] + [repr(float(v)) for v in lake],
                           capture_output=True, text=True, timeout=300, env=env)
        if r.returncode < 0 or r.returncode in (134, 139):                      # the worker died on the GPU: nothing more is started there
            pytest.exit(f"wall_still_worker {case} {cols}x{rows} ended with {r.returncode}: {r.stdout}{r.stderr}", returncode=3)
        assert r.returncode == 0, r.stdout + r.stderr
        print(f"wall={wall} skip={skip} rseg={rseg}: {r.stdout.strip()}")
        _runs[key] = dict(np.load(out))
    return _runs[key]


def same_bits(a, b, what):
    assert int(a["iterations"]) == int(b["iterations"]), what
    assert a["t"].view(np.uint64) == b["t"].view(np.uint64), what
    assert a["dt"].view(np.uint64) == b["dt"].view(np.uint64), what
    x, y = a["state"].view(np.uint64), b["state"].view(np.uint64)
    assert x.shape == y.shape
    bad = np.argwhere(x != y)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[:5].tolist()}"


def reference_is_no_full_march(ref, new, cols):
    """The precondition (see above)."""
    assert int(ref["launches"]) < int(ref["iterations"]), "the reference took no pairs"
    assert int(ref["wall_still"].max()) == 0, "HP_PAIR_WALL=0 recorded rows beside the ring"
    if cols >= 302:
        assert int(ref["skipped"].max()) > 0, f"HP_PAIR_WALL=0 skipped no interior tile: {ref['skipped'].tolist()}"
    else:
        assert int(new["skipped"].max()) > 0, f"neither run skipped a tile: {new['skipped'].tolist()}"


# 122 x 52: two windows wide, both beside the ring; 242 x 100 and 302 x 100: interior windows between them; 242 x 89 at 8 rows a tile: bands of 10 or 11
# rows, so a partial tile ends every band; tiles of two rows, the smallest there are, in a box with four updated rows: the tiles whose
# stencils reach the bottom ring row and the top one are neighbours (a box with two updated rows, where they are one tile, takes no
# pairs at all: 12 launches for 12 iterations with every setting)
SHAPES = [(122, 52, None), (302, 100, None), (242, 100, None), (242, 89, 8), (122, 6, 2)]
LAKES = [(10.0, 0.0), (1.0, 0.0), (2.5, 0.5)]


# (S-DAM's two levels at every shape, a lake over a raised bed at one)
CASES = [(s, l) for s in SHAPES for l in LAKES[:2]] + [(SHAPES[1], LAKES[2])]


@pytest.mark.parametrize("shape,lake", CASES, ids=lambda v: "x".join(str(w) for w in v))
def test_still_lake_inside_walls(shape, lake, tmp_path_factory):
    cols, rows, rseg = shape
    new = run(tmp_path_factory, "lake", cols, rows, rseg=rseg, lake=lake)
    ref = run(tmp_path_factory, "lake", cols, rows, wall=0, rseg=rseg, lake=lake)
    full = run(tmp_path_factory, "lake", cols, rows, skip=0, rseg=rseg, lake=lake)
    reference_is_no_full_march(ref, new, cols)
    assert int(full["skipped"].max()) == 0 and int(full["wall_still"].max()) == 0       # HP_PAIR_SKIP=0 switches both off
    # the lake is still: the first pair records the rows beside the ring, and a pair that follows a pair skips them (the batch of three
    # begins with one; a single iteration in between, as odd batches bring, drops the records)
    assert int(new["wall_still"].min()) > 0 and int(new["wall_skipped"].max()) > 0, (new["wall_still"].tolist(), new["wall_skipped"].tolist())
    same_bits(new, ref, "HP_PAIR_WALL=0")
    same_bits(new, full, "HP_PAIR_SKIP=0")
    st0 = new["state"][1:-1, 1:-1]
    assert (st0[..., 0] == lake[0]).all() and (st0[..., 2:].view(np.uint64) == 0).all()     # (and it is still the lake it was)


def test_surviving_wall_term_is_never_taken(tmp_path_factory):
    new = run(tmp_path_factory, "lake", 302, 100, lake=SURVIVING)
    ref = run(tmp_path_factory, "lake", 302, 100, wall=0, lake=SURVIVING)
    full = run(tmp_path_factory, "lake", 302, 100, skip=0, lake=SURVIVING)
    reference_is_no_full_march(ref, new, 302)
    same_bits(new, ref, "HP_PAIR_WALL=0")
    same_bits(new, full, "HP_PAIR_SKIP=0")
    moved = new["state"][1:-1, 1:-1, 2:].view(np.uint64) != 0
    assert moved.any(), "the lake did not start to move at its walls: not the pair this test is about"
    assert int(new["wall_still"].max()) == 0, new["wall_still"].tolist()                 # no row beside the ring was ever marked


# (542 columns: nine windows, the dam in the middle one -- the reference skips in the third and the seventh, whose neighbours are neither
# ring windows nor the dam's, until the front is there)
@pytest.mark.parametrize("cols,rows", [(122, 52), (542, 100)])
def test_dam_break_reaches_the_walls(cols, rows, tmp_path_factory):
    new = run(tmp_path_factory, "dam", cols, rows)
    ref = run(tmp_path_factory, "dam", cols, rows, wall=0)
    same_bits(new, ref, "HP_PAIR_WALL=0")
    if cols > 122:
        # the outer windows are still at first and skipped; the front has reached every window and both walls by the end: nothing beside
        # the ring is still any more (at 122 columns both windows hold the dam itself from the start)
        assert int(ref["skipped"].max()) > 0, ref["skipped"].tolist()
        assert int(new["wall_skipped"][0]) > 0, new["wall_skipped"].tolist()
        assert int(new["wall_skipped"][-1]) == 0 and int(new["wall_still"][-1]) == 0, (new["wall_skipped"].tolist(), new["wall_still"].tolist())
    else:
        assert int(ref["launches"]) < int(ref["iterations"])
        assert int(new["wall_still"].max()) == 0, new["wall_still"].tolist()


@pytest.mark.parametrize("case", ["wet_ring", "two_beds", "disabled", "negzero"])
def test_ring_that_is_not_one_wall(case, tmp_path_factory):
    lake = (1.0, 0.0)
    new = run(tmp_path_factory, case, 302, 100, lake=lake)
    ref = run(tmp_path_factory, case, 302, 100, wall=0, lake=lake)
    reference_is_no_full_march(ref, new, 302)
    same_bits(new, ref, "HP_PAIR_WALL=0")
    if case != "disabled":
        # the windows that hold the odd cells are not taken: fewer rows beside the ring are recorded than in the plain lake
        # (a ring cell whose Zmax alone says disabled is a wall to its neighbours like any other: taken or not, the same bits)
        plain = run(tmp_path_factory, "lake", 302, 100, lake=lake)
        assert int(new["wall_still"].max()) < int(plain["wall_still"].max()), (new["wall_still"].tolist(), plain["wall_still"].tolist())


@pytest.mark.parametrize("case", ["upload", "upload_mound", "bed_apply", "links"])
def test_host_writes_drop_the_records(case, tmp_path_factory):
    lake = (1.0, 0.0)
    new = run(tmp_path_factory, case, 302, 100, lake=lake)
    ref = run(tmp_path_factory, case, 302, 100, wall=0, lake=lake)
    reference_is_no_full_march(ref, new, 302)
    same_bits(new, ref, "HP_PAIR_WALL=0")
    # the first pair behind the write reads no records: it skips nothing, beside the ring or elsewhere (links: the batch behind the clear)
    k = 2 if case == "links" else 1
    assert int(new["skipped"][k]) == 0 and int(new["wall_skipped"][k]) == 0, (new["skipped"].tolist(), new["wall_skipped"].tolist())
    plain = run(tmp_path_factory, "lake", 302, 100, lake=lake)
    assert int(plain["wall_skipped"][1]) > 0                                             # (without the write it does)
