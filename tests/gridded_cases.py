"""Gridded boundaries away from offset 0 and whole-cell resolutions: the table of offsets, resolutions and grid sizes, the NumPy
restatement of the lookup, and the scene, shared by tests/test_gridded_lookup.py (CPU), tests/test_gpu_gridded_lookup.py and its
worker tests/gridded_lookup_worker.py.  No test in here.

The lookup (Boundaries/CLBoundaries.clc:231-234), T being the domain's precision:
    col = floor(((T)x * dx - off_x) / resolution),  row = floor(((T)gy * dx - off_y) / resolution)
    rate = grids[(grid_rows * grid_cols) * slice + grid_cols * row + col]
`indices` evaluates it at EVERY coordinate with NumPy scalars of type T (each operation rounded once, nothing fused)."""
import numpy as np

COLS, ROWS = 190, 101          # three 62-column windows and a remainder, several tiles, neither a multiple of 8 (Q9 cuts both)
DXS = (40.0, 0.3)              # timesteps above a second (the hydrological gate opens on every iteration) / not representable
RES_FUSED = (64.0, 66.7)       # in cells: on the fusion threshold, and uneven above it
RES_FINE = (63.99, 8.0, 7.3)   # below the threshold by a hair, and the fine grids of the stand-alone pass
RESOLUTIONS = RES_FUSED + RES_FINE
DEFINITIONS = (0, 2)           # rain intensity, mass flux
SLICES, INTERVAL, T0, DT0 = 3, 45.0, 70.0, 2.0
PLAN = (1, 2, "download", 5, 4)   # odd and even batches, a batch's unfused last iteration, a cold start behind the download


def offsets(dx, res):
    """(off_x, off_y): the control, the largest the cover check allows (row and column 0 index -1), and three uneven ones."""
    return ((0.0, 0.0), (dx, dx), (-0.37 * res, -0.61 * res), (dx / 2, -res), (-res, dx / 2))


def indices(real, n, dx, off, res):
    """The lookup's index (as T, floor's result) at coordinates 0 .. n - 1."""
    i = np.arange(n).astype(real)
    with np.errstate(all="ignore"):
        return np.floor((i * real(dx) - real(off)) / real(res))


def covers(real, n, dx, off, res, cells):
    """Every interior coordinate 1 .. n - 2 indexes inside [0, cells)."""
    idx = indices(real, n, dx, off, res)[1:n - 1]
    return bool((idx >= 0).all() and (idx.astype(np.float64) < float(cells)).all())


def smallest_grid(real, dx, res, off_x, off_y, cols=COLS, rows=ROWS):
    """(grid_rows, grid_cols) of the smallest grid that covers the interior cells in precision T."""
    cx, cy = indices(real, cols, dx, off_x, res)[1:cols - 1], indices(real, rows, dx, off_y, res)[1:rows - 1]
    assert cx.min() >= 0 and cy.min() >= 0, (dx, res, off_x, off_y)
    return int(cy.max()) + 1, int(cx.max()) + 1


def table(dx, real, resolutions=RESOLUTIONS, cols=COLS, rows=ROWS):
    """The rows: (label, resolution, off_x, off_y, grid_rows, grid_cols) -- every offset at every resolution, on the smallest grid
    the cover check accepts and on that grid with one more row and column."""
    out = []
    for rc in resolutions:
        res = rc * dx
        for k, (ox, oy) in enumerate(offsets(dx, res)):
            gr, gc = smallest_grid(real, dx, res, ox, oy, cols, rows)
            for extra in (0, 1):
                out.append((f"res{rc:g}-off{k}-{'min' if not extra else 'plus1'}", res, ox, oy, gr + extra, gc + extra))
    return out


def rates(definition, entries, grid_rows, grid_cols, real, seed=11):
    """A distinct rate per grid cell and slice (a wrong cell cannot give the right value), shuffled by a seeded generator.
    Rain in mm/h up to 800; the mass flux scaled so that a cell of dx = 40 m gains millimetres, as the rain does."""
    n = entries * grid_rows * grid_cols
    v = (1.0 + np.random.default_rng(seed + 7 * definition).permutation(n)) / n
    g = (v * (800.0 if definition == 0 else 800.0 / 3600000.0 * 1600.0)).reshape(entries, grid_rows, grid_cols).astype(real)
    assert len(np.unique(g)) == n
    return g


def increment(real, definition, grids, slice_, dx, res, off_x, off_y, t_hydro, cols=COLS, rows=ROWS, row_offset=0):
    """The level increment of every cell [rows, cols] (no range test: the caller masks), row, column and slice per cell in T."""
    col = indices(real, cols, dx, off_x, res).astype(np.int64)
    row = indices(real, row_offset + rows, dx, off_y, res).astype(np.int64)[row_offset:]
    ok = (row >= 0)[:, None] & (col >= 0)[None, :] & (row < grids.shape[1])[:, None] & (col < grids.shape[2])[None, :]
    rate = grids[slice_][np.clip(row, 0, grids.shape[1] - 1)[:, None], np.clip(col, 0, grids.shape[2] - 1)[None, :]]
    if definition == 0:
        inc = rate / real(3600000.0) * real(t_hydro)
    else:
        inc = rate / (real(dx) * real(dx)) * real(t_hydro)
    return inc.astype(real), ok


def scene(real, cols=COLS, rows=ROWS):
    """syn.s_rough lowered to mostly dry land with pools at rest, the edge ring zeroed (tests/two_step_worker.py's rain scenarios)."""
    from hipims_mi import synthetic as syn
    st, bed, man = syn.s_rough(cols, rows, dtype=np.float64, manning=None)
    st[..., 0] = np.maximum(bed, st[..., 0] - 0.6); st[..., 1] = st[..., 0]
    st[..., 2:] = 0
    st[0] = st[-1] = 0; st[:, 0] = st[:, -1] = 0
    return st.astype(real), bed.astype(real), man.astype(real)
