"""The moving bed on the GPU: the domain and the runs of tests/test_gpu_bed_shapes.py, importable (the test's in-process cases)
and a program of its own where an environment variable is read once: `bed_shapes_worker.py <case>` runs the round-trip comparison
of one case with HP_TWO_STEP=1 set by the caller and demands that iteration pairs really ran.

The domain: 200 columns x 96 rows.  Water at level 3 m west of a wall of bed 5 m, 4 columns thick over all 96 rows (columns
100-103); everything east dry on an undulating bed; closed edges, so rows 0 and 95 are walls; one disabled cell inside the wall.
Shape A: all 384 wall cells to 0.5 m (more than one 256-thread block; it holds the wall-row cells and the disabled cell, so the
skip path runs), from 2 s to 12 s in 4 knots.  Shape B: a 2-cell barrier in the dry part, 0 -> 1 -> 0.4, from 3 s to 14 s.
The clock starts at T0 = 60 s (hp_set_time) and the series' times are counted from there: in its first 60 s a run's timestep is
capped at 0.1 s (the reference's early limit, CLDynamicTimestep.clh:24-29), and twelve batches of 7 or 8 such steps end at 9 s, before
the series do.  With 3 m cells a batch is 1.4 to 2.2 s (the CPU oracle on this domain): the first apply comes before 2 s, four after 14 s."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd")]
import numpy as np  # noqa: E402

import hipims_mi as hp  # noqa: E402
from hipims_mi import frontend, synthetic as syn  # noqa: E402

COLS, ROWS, DX, T0 = 200, 96, 3.0, 60.0
WALL = range(100, 104)
ROUNDS = 12
CASES = {                                             # scheme, math mode, precision
    "godunov-fast-f64": (hp.SCHEME_GODUNOV, hp.MATH_FAST, "f64"),
    "godunov-fast-f32": (hp.SCHEME_GODUNOV, hp.MATH_FAST, "f32"),
    "godunov-strict-f64": (hp.SCHEME_GODUNOV, hp.MATH_STRICT, "f64"),
    "muscl-fast-f64": (hp.SCHEME_MUSCL_HANCOCK, hp.MATH_FAST, "f64"),
    "inertial-fast-f64": (hp.SCHEME_INERTIAL, hp.MATH_FAST, "f64"),
}


def arrays(real=np.float64):
    y, x = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    bed = syn.round4(0.2 * np.sin(2 * np.pi * x / 37.0) * np.cos(2 * np.pi * y / 29.0) + 0.3)
    bed[:, :WALL[0]] = 0.0
    bed[:, WALL[0]:WALL[-1] + 1] = 5.0
    st = np.zeros((ROWS, COLS, 4))
    st[..., 0] = bed
    st[:, :WALL[0], 0] = 3.0
    st[..., 1] = st[..., 0]
    syn._walls(st, bed)
    st[40, 101, 1] = -9999.0                          # a disabled cell inside the wall
    return st.astype(real), bed.astype(real), np.full((ROWS, COLS), 0.03, real)


def shapes():
    a = [y * COLS + x for y in range(ROWS) for x in WALL]
    b = [(150, 30), (151, 30)]
    return [(a, 0.5, [(T0 + 2.0, 0.0), (T0 + 5.0, 0.2), (T0 + 9.0, 0.7), (T0 + 12.0, 1.0)]),
            (b, [1.5, 1.25], [(T0 + 3.0, 0.0), (T0 + 6.0, 1.0), (T0 + 14.0, 0.4)])]


def make(case, **kw):
    scheme, math_mode, precision = CASES[case]
    dom = hp.Domain(COLS, ROWS, dx=DX, scheme=scheme, precision=precision, math_mode=math_mode, **kw)
    st, bed, man = arrays(dom.real)
    dom.upload(st, bed, man)
    dom.set_time(T0)
    dom.set_target_time(1e9)
    dom.update_timestep()
    return dom


def add_shapes(dom):
    for cells, target, series in shapes():
        dom.bed_shape_add(cells, target, series)


def host_shapes(bed):
    ref = frontend.BedShapes(ROWS, COLS)
    for cells, target, series in shapes():
        ref.add(cells, target, series, bed=bed)
    return ref


def round_trip(b, ref):
    """Run B's half of a round: what hp_bed_apply replaces.  Returns what BedShapes.apply changed."""
    b.sync()
    t = b.read_scalars()["time"]
    st, bed = b.download(), b.download(hp.ARRAY_BED)
    changed = ref.apply(st, bed, t)
    b.upload(bed=bed)
    b.upload(state=st)
    return changed, t


def same(a, b):
    return bool(np.array_equal(a.download(), b.download()) and np.array_equal(a.download(hp.ARRAY_BED), b.download(hp.ARRAY_BED))
                and a.read_scalars() == b.read_scalars())


def compare_with_the_round_trip(case, rounds=ROUNDS, batches=(7, 8)):
    """-> one dict per round: same, changed (A's bed_info), want (BedShapes.apply's count), t."""
    a, b = make(case), make(case)
    add_shapes(a)
    ref = host_shapes(b.download(hp.ARRAY_BED))
    out = []
    for r in range(rounds):
        n = batches[r % len(batches)]
        a.step_batch(n)
        a.bed_apply()
        b.step_batch(n)
        want, t = round_trip(b, ref)
        info = a.bed_info()
        out.append(dict(same=same(a, b), changed=info["changed_last"], want=want, t=t, t_last=info["t_last"], applies=info["applies"]))
    pairs = (a.pair_stats()["pairs"], b.pair_stats()["pairs"])
    bed = a.download(hp.ARRAY_BED)
    a.close(); b.close()
    return out, pairs, bed


if __name__ == "__main__":
    case = sys.argv[1]
    assert os.environ.get("HP_TWO_STEP") == "1"
    rounds, pairs, _ = compare_with_the_round_trip(case)
    ok = all(r["same"] and r["changed"] == r["want"] for r in rounds) and pairs[0] > 0 and pairs[1] > 0
    print(case, "identical to the round trip in every round", all(r["same"] for r in rounds), "counts", [(r["changed"], r["want"]) for r in rounds],
          "pairs ran", pairs, flush=True)
    sys.exit(0 if ok else 1)
