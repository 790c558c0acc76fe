"""Random host-call sequences and their oracle twin (shared by host_calls_worker.py, test_gpu_host_calls.py and test_host_calls_cpu.py).

The engine's correctness between launches rests on host-side flags (m1_valid, other_stale, use_alt, rings_differ, need_full_reduce,
spec_now ...) that every entry point changes (most of them through the events of csrc/hp_facts.hpp).  `make_sequence(seed, leg)` draws a small configuration and 8-20 host
calls in any order -- batches on both sides of SPEC_MIN and of the tuner's 12, split steps, time-control calls, full / partial /
block-wise state uploads, bed and Manning uploads, boundaries added and cleared mid-run, checkpoints with anything in between,
observer samples, downloads -- and `execute(seq, sim)` runs them on anything with the small surface of `EngineSim` / `OracleTwin`.

The oracle twin.  `run_on_oracle(seq)` executes the LINEARISED sequence on oracle.OracleSim: a split step is run(1), an observer sample
is nothing.  The oracle cannot go back, so at a `restore` the twin builds a second oracle and replays, from the start, every call made
before the matching `save`; the calls made between save and restore are left out, except those a checkpoint does not carry
(hp_state_save keeps both state buffers, the scalars -- time, timestep, target time, counters --, the CFL slot block and the observers'
counts; the bed, the Manning map and the boundary list are NOT part of it): those are applied at the restore point.  That is
equivalent, because the boundaries' series are functions of absolute time and the bed / Manning arrays act from the next iteration on.

What the oracle cannot do.  swe_oracle.c has no partial upload (its upload writes both buffers), no way to drop its boundaries and no
call that sets the time: `rows2`, `blocks`, `clear` and `set_time` are drawn for the "fast" leg only, whose bar is the engine's own run
with pairs off; a sequence that contains one of them has `oracle_ok == False` and is held to that bar alone.
"""
import hashlib

import numpy as np

GODUNOV, MUSCL, INERTIAL = 0, 1, 2                     # hipims_mi.SCHEME_* == oracle.GODUNOV ...
UNIFORM_RAIN, UNIFORM_LOSS, GRIDDED_RAIN, GRIDDED_MASS_FLUX = 0, 1, 0, 2
QUIRKS_REFERENCE, Q6_MUSCL_SERIAL = 15, 4              # oracle's masks
SPEC_MIN = 8                                           # hp_engine.hip
MAX_ITERATIONS = 200
COLS, ROWS = (5, 33, 64, 65, 130, 257), (5, 6, 19, 37, 64, 101)
BATCHES = (1, 2, 3, 7, 8, 9, 12, 20, 33)
LEGS = ("strict", "spec", "fast")
# first seed of each leg: chosen so that the oracle's own run stays finite on at least 95 % of the 120 seeds (test_host_calls_cpu.py)
SEED_BASE = {"strict": 11000, "spec": 13000, "fast": 15000}
SEEDS_PER_LEG, CHUNK = 120, 30
ORACLE_LESS = ("rows2", "blocks", "clear", "set_time")
BOUNDARY_OPS = ("uniform", "gridded", "cell", "clear")
PATTERNS = ("split_after_boundary_pairs", "boundary_change_in_checkpoint", "speculation_after_short_pairs", "blocks_then_batch")
OP_KINDS = ("batch", "split", "target", "force_dt", "reset", "update", "set_time", "upload", "rows2", "blocks", "bed", "manning",
            "uniform_rain", "uniform_loss", "gridded_rain", "mass_flux", "cell", "clear", "save", "restore", "sample", "download")


def _synthetic():
    from hipims_mi import synthetic as syn
    return syn


def rough_with_nulls(cols, rows):
    st, bed, man = _synthetic().s_rough(cols, rows, manning=None, seed=31, pool_level=0.1)       # (a low pool: dry ground on every hill)
    for y, x in ((5, 7), (20, 40), (30, 12)):
        st[y, x, 0] = -9999.0; st[y, x, 1] = -9999.0; st[y, x, 2:] = 0
    bed[20, 40] = -9999.0
    return st, bed, man


def make_sequence(seed, leg="fast"):
    """dict(cfg=..., ops=[(kind, args...)], patterns={name: count}, oracle_ok, iterations) -- a pure function of (seed, leg)."""
    assert leg in LEGS
    syn = _synthetic()
    rng = np.random.default_rng(seed)
    r = float(rng.random())
    scheme = GODUNOV if r < 0.7 else MUSCL if r < 0.85 else INERTIAL
    precision = "f64" if (rng.random() < 0.65 or leg == "spec") else "f32"
    real = np.float64 if precision == "f64" else np.float32
    cols, rows = int(rng.choice(COLS)), int(rng.choice(ROWS))
    dx = float(rng.choice([1.0, 2.0, 0.5]))
    terrain = "rough" if rng.random() < 0.75 else "dam"
    if terrain == "rough":
        st, bed, man = syn.s_rough(cols, rows, dtype=real, seed=int(rng.integers(1, 10 ** 6)), amplitude=float(rng.uniform(0.1, 0.8)),
                                   pool_level=float(rng.uniform(-0.2, 0.5)), manning=None if rng.random() < 0.6 else 0.035)
        for _ in range(int(rng.integers(1, 5))):             # a few null cells (mask style, now and then DEM-nodata style): Q3-untouched cells exist
            y, x = int(rng.integers(1, rows - 1)), int(rng.integers(1, cols - 1))
            st[y, x, 0] = -9999.0; st[y, x, 1] = -9999.0; st[y, x, 2:] = 0
            if rng.random() < 0.4:
                bed[y, x] = -9999.0
    else:
        st, bed, man = syn.s_dam(cols, rows, dtype=real, wet_right=bool(rng.random() < 0.5))
    if scheme == INERTIAL:                                   # gentler discharges: the scheme is not positivity preserving
        st[..., 2:] *= real(0.1)
        if terrain == "dam":
            st, bed, man = syn.s_dam(cols, rows, dtype=real, levels=(1.2, 1.0))
    friction = bool(rng.random() < 0.75)
    with_bdy = scheme != MUSCL and rng.random() < (0.65 if leg == "fast" else 0.5)     # (MUSCL-Hancock never applies them, quirk Q8)
    dynamic = bool(with_bdy or rng.random() < 0.85)          # a fixed timestep only without boundaries
    fixed_dt = float(rng.choice([0.002, 0.004])) * dx
    observers = bool(rng.random() < 0.3)
    cfg = dict(seed=seed, leg=leg, scheme=scheme, precision=precision, cols=cols, rows=rows, dx=dx, terrain=terrain, st=st, bed=bed, man=man,
               friction=friction, dynamic=dynamic, fixed_dt=fixed_dt, observers=observers, math="fast" if leg == "fast" else "strict")

    def uniform(definition):
        if definition == UNIFORM_RAIN:
            iv = float(rng.choice([0.7, 5.0]))
            return ("uniform", UNIFORM_RAIN, np.array([[0.0, rng.uniform(50, 900)], [iv, rng.uniform(0, 300)], [2 * iv, rng.uniform(0, 100)], [3 * iv, 0.0]]), iv, 3 * iv)
        return ("uniform", UNIFORM_LOSS, np.array([[0.0, rng.uniform(100, 2000)], [100.0, 5.0]]), 100.0, 100.0)

    def gridded(definition):
        res = 64.0 * dx                                      # coarse: rides in the flux kernel (fusable)
        gr, gc = int(np.ceil(rows * dx / res)) + 1, int(np.ceil(cols * dx / res)) + 1
        scale = 1.0 if definition == GRIDDED_RAIN else 1e-4
        return ("gridded", definition, rng.uniform(0.0, 600.0, (3, gr, gc)) * scale, res, float(rng.choice([0.5, 3.0])))

    def cell():
        ids = np.unique(np.array([int(rng.integers(1, rows - 1)) * cols + int(rng.integers(1, cols - 1)) for _ in range(4)], np.uint64))
        series = np.array([[0.0, 0.3, 0.05, -0.02], [50.0, 0.5, 0.08, 0.03], [100.0, 0.2, 0.0, 0.0]])
        return ("cell", int(rng.integers(0, 3)), int(rng.integers(0, 4)), ids, series, 50.0, 100.0)

    def boundary():
        k = float(rng.random())
        return uniform(UNIFORM_RAIN) if k < 0.35 else uniform(UNIFORM_LOSS) if k < 0.55 else gridded(GRIDDED_RAIN) if k < 0.75 else \
            gridded(GRIDDED_MASS_FLUX) if k < 0.9 else cell()

    ops = []
    if with_bdy:
        for _ in range(int(rng.integers(1, 3))):
            b = boundary()
            ops.append(b if b[0] != "cell" or rng.random() < 0.3 else uniform(UNIFORM_RAIN))
    kinds = ["batch"] * 6 + ["split"] * 2 + ["target", "force_dt", "reset", "update", "upload", "bed", "manning", "save", "save", "restore", "restore",
                                             "sample", "download", "download"]
    if with_bdy:
        kinds += ["boundary"] * 2
    if leg == "fast" and rng.random() < 0.6:                 # (the rest of the leg's seeds stay within what the oracle can follow)
        kinds += ["rows2", "blocks", "blocks", "set_time"] + (["clear"] if with_bdy else [])
    left, saved = MAX_ITERATIONS, False
    n_ops = int(rng.integers(8, 21))
    while len(ops) < n_ops + (2 if with_bdy else 0):
        kind = str(rng.choice(kinds))
        if kind == "batch":
            n = int(min(left, rng.choice(BATCHES)))
            if n < 1:
                continue
            left -= n
            ops.append(("batch", n))
        elif kind == "split":
            k = int(min(left, rng.integers(1, 4)))
            if k < 1:
                continue
            left -= k
            ops.append(("split", k))
        elif kind == "target":
            ops.append(("target", float(rng.choice([0.05, 0.5, 5.0, 1e9]))))
        elif kind == "force_dt":
            ops.append(("force_dt", float(rng.choice([0.001, 0.0005])) * dx))
        elif kind == "set_time":
            ops.append(("set_time", float(rng.choice([0.25, 1.0]))))
        elif kind in ("upload", "bed", "manning"):
            ops.append((kind, float(rng.uniform(0.005, 0.05))))
        elif kind == "rows2":
            ops.append(("rows2", int(rng.integers(0, rows - 1)), bool(rng.random() < 0.6)))      # (row0, interior columns only)
        elif kind == "blocks":
            cuts, y = [], 0
            while y < rows:
                h = int(min(rows - y, rng.integers(1, max(2, rows // 2))))
                cuts.append(h); y += h
            ops.append(("blocks", tuple(cuts), float(rng.choice([0.0, 0.02]))))
        elif kind == "boundary":
            ops.append(boundary())
        elif kind == "save":
            saved = True
            ops.append(("save",))
        elif kind == "restore":
            if not saved:
                continue
            ops.append(("restore",))
        else:
            ops.append((kind,))
    ops.append(("download",))
    seq = dict(cfg=cfg, ops=ops, iterations=MAX_ITERATIONS - left, oracle_ok=not any(o[0] in ORACLE_LESS for o in ops))
    seq["patterns"] = count_patterns(seq)
    return seq


def op_name(op):
    """The operation kind as OP_KINDS names it (the four area boundaries apart)."""
    if op[0] == "uniform":
        return "uniform_rain" if op[1] == UNIFORM_RAIN else "uniform_loss"
    if op[0] == "gridded":
        return "gridded_rain" if op[1] == GRIDDED_RAIN else "mass_flux"
    return op[0]


def count_patterns(seq):
    """How often the four call patterns behind the round-6 findings occur, from the operations alone (no run needed)."""
    cfg, found = seq["cfg"], dict.fromkeys(PATTERNS, 0)
    pairs_cfg = cfg["scheme"] == GODUNOV and cfg["dynamic"]
    area = cells = 0                                         # boundaries attached now
    last_iter = None                                         # the last op that ran iterations (downloads and samples do not count)
    save_at, changed_since_save, blocks_pending = None, False, False
    for op in seq["ops"]:
        kind = op[0]
        if kind in ("uniform", "gridded"):
            area += 1
        elif kind == "cell":
            cells += 1
        elif kind == "clear":
            area = cells = 0
        if kind in BOUNDARY_OPS and save_at is not None:
            changed_since_save = True
        if kind == "save":
            save_at, changed_since_save = (area, cells), False
        elif kind == "restore":
            found["boundary_change_in_checkpoint"] += int(changed_since_save)
            changed_since_save = False                       # (the boundary list is not rolled back: area / cells stay)
        elif kind == "blocks":
            blocks_pending = True
        elif kind == "upload":
            blocks_pending = False
        elif kind == "split":
            if last_iter and last_iter[0] == "batch" and last_iter[1] >= 2 and last_iter[2] and cfg["leg"] == "fast" and pairs_cfg:
                found["split_after_boundary_pairs"] += 1
            last_iter = ("split", op[1], False)
        elif kind == "batch":
            if blocks_pending:
                found["blocks_then_batch"] += 1
                blocks_pending = False
            if (cfg["leg"] == "spec" and pairs_cfg and area + cells == 0 and op[1] >= SPEC_MIN and last_iter and last_iter[0] == "batch"
                    and 2 <= last_iter[1] < SPEC_MIN and last_iter[3]):
                found["speculation_after_short_pairs"] += 1
            last_iter = ("batch", op[1], area > 0 and cells == 0, area + cells == 0)
        elif kind not in ("download", "sample"):
            last_iter = None
    return found


# ---- the two things a sequence runs on -----------------------------------------------------------------------------------------------
class EngineSim:
    """The HIP engine behind the surface `execute` drives."""

    def __init__(self, cfg):
        import hipims_mi as hp
        import oracle
        self.hp, self.cfg = hp, cfg
        self.dom = hp.Domain(cfg["cols"], cfg["rows"], dx=cfg["dx"], scheme=cfg["scheme"], precision=cfg["precision"],
                             quirks=oracle.quirks_to_engine(QUIRKS_REFERENCE), friction=cfg["friction"], dynamic_dt=cfg["dynamic"],
                             dt_fixed=cfg["fixed_dt"], dt_initial=cfg["fixed_dt"] if not cfg["dynamic"] else 0.001,
                             math_mode=hp.MATH_STRICT if cfg["math"] == "strict" else hp.MATH_FAST)
        self.bed = None
        self.pairs_by_batch = []

    def upload(self, state=None, bed=None, manning=None):
        if bed is not None:
            self.bed = np.array(bed)
        self.dom.upload(state, bed, manning)

    def observers(self):
        cfg, dom = self.cfg, self.dom
        dom.peaks_enable(list(self.hp.PEAK_CODES))
        dom.probes_enable(gauges=[(cfg["cols"] // 2, cfg["rows"] // 2), (1, 1)])
        dom.zones_enable((np.arange(cfg["rows"] * cfg["cols"]).reshape(cfg["rows"], cfg["cols"]) % 3).astype(np.uint16), zone_count=2)

    def sample(self):
        if self.cfg["observers"]:
            self.dom.peaks_sample(); self.dom.probes_sample(); self.dom.zones_sample()

    def download(self):
        return self.dom.download()

    def time(self):
        return self.dom.read_scalars()["time"]

    def step_batch(self, n):
        before = self.dom.pair_stats()["pairs"]
        self.dom.step_batch(n)
        self.pairs_by_batch.append(self.dom.pair_stats()["pairs"] - before)

    def split(self):
        self.dom.step_begin(); self.dom.step_end()

    def set_target(self, t): self.dom.set_target_time(t)
    def force_dt(self, dt): self.dom.force_timestep(dt)
    def reset_counters(self): self.dom.reset_counters()
    def update_timestep(self): self.dom.update_timestep()
    def set_time(self, t): self.dom.set_time(t)
    def upload_rows(self, patch, row0): self.dom.upload_rows(patch, row0)
    def add_uniform(self, *a): self.dom.add_uniform(*a)
    def add_gridded(self, *a): self.dom.add_gridded(*a)
    def add_cell(self, *a): self.dom.add_cell(*a)
    def clear_boundaries(self): self.dom.clear_boundaries()
    def save(self): self.dom.state_save()
    def restore(self): self.dom.state_restore()

    def scalars(self):
        sc = self.dom.read_scalars()
        return (sc["time"], sc["timestep"], sc["time_hydrological"], sc["batch_successful"], sc["batch_skipped"])

    def close(self):
        self.dom.close()


class OracleTwin:
    """oracle.OracleSim with a memory: every call is logged, and a restore replays the log on a second oracle (module docstring)."""
    CARRIED_OVER = ("add_uniform", "add_gridded", "add_cell")        # ... and uploads of the bed / the Manning map

    def __init__(self, cfg):
        self.cfg, self.log, self.mark, self.bed = cfg, [], None, None
        self.sim = self._fresh()
        self.rebuilds = 0

    def _fresh(self):
        import oracle
        cfg = self.cfg
        quirks = QUIRKS_REFERENCE & ~(Q6_MUSCL_SERIAL if cfg["scheme"] == MUSCL else 0)        # (the engine is always snapshot order)
        return oracle.OracleSim(cfg["cols"], cfg["rows"], dx=cfg["dx"], scheme=cfg["scheme"], precision=cfg["precision"], quirks=quirks,
                                friction=cfg["friction"], dynamic_dt=cfg["dynamic"], fixed_dt=cfg["fixed_dt"],
                                dt_initial=cfg["fixed_dt"] if not cfg["dynamic"] else 0.001)

    def _call(self, name, *args, **kw):
        self.log.append((name, args, kw))
        getattr(self.sim, name)(*args, **kw)

    def upload(self, state=None, bed=None, manning=None):
        if bed is not None:
            self.bed = np.array(bed)
        for key, arr in (("bed", bed), ("manning", manning), ("state", state)):                 # one array per entry: each is kept or dropped on its own
            if arr is not None:
                self._call("upload", **{key: np.array(arr)})

    def observers(self): pass
    def sample(self): pass
    def download(self): return self.sim.download()
    def time(self): return self.sim.scalars()["t"]
    def step_batch(self, n): self._call("run", n)
    def split(self): self._call("run", 1)
    def set_target(self, t): self._call("set_target", t)
    def force_dt(self, dt): self._call("force_dt", dt)
    def reset_counters(self): self._call("reset_counters")
    def update_timestep(self): self._call("update_timestep")
    def add_uniform(self, *a): self._call("add_uniform", *a)
    def add_gridded(self, *a): self._call("add_gridded", *a)
    def add_cell(self, *a): self._call("add_cell", *a)

    def set_time(self, t): raise NotImplementedError("the oracle has no call that sets the time")
    def upload_rows(self, patch, row0): raise NotImplementedError("the oracle has no partial upload")
    def clear_boundaries(self): raise NotImplementedError("the oracle cannot drop its boundaries")

    def save(self):
        self.mark = len(self.log)

    def restore(self):
        kept = [c for c in self.log[self.mark:] if c[0] in self.CARRIED_OVER or (c[0] == "upload" and "state" not in c[2])]
        self.log = self.log[:self.mark] + kept
        self.sim = self._fresh()
        self.rebuilds += 1
        for name, args, kw in self.log:
            getattr(self.sim, name)(*args, **kw)

    def scalars(self):
        sc = self.sim.scalars()
        return (sc["t"], sc["dt"], sc["t_hydro"], sc["batch_ok"], sc["batch_skipped"])

    def close(self):
        self.sim = None


def execute(seq, sim, extra=None, point=None):
    """Run the sequence on `sim`; dict(points=[state at every download], scalars, finite).  `extra(op, sim)` runs the operation kinds
    this module does not draw and `point(sim)` is what a download compares, its first element the state (host_calls_actors.py)."""
    cfg = seq["cfg"]
    rows, cols, real = cfg["rows"], cfg["cols"], cfg["st"].dtype.type
    live = cfg["st"][..., 1] > -9000                          # (null cells stay what they are)
    sim.upload(cfg["st"], cfg["bed"], cfg["man"])
    sim.set_target(1e9)
    if cfg["observers"]:
        sim.observers()
    points, manning_uniform = [], bool(cfg["man"].std() == 0)
    for op in seq["ops"]:
        kind = op[0]
        if kind == "batch":
            sim.step_batch(op[1])
        elif kind == "split":
            for _ in range(op[1]):
                sim.split()
        elif kind == "target":
            sim.set_target(op[1] if op[1] > 1e8 else sim.time() + op[1])
            sim.update_timestep()
        elif kind == "force_dt":
            sim.force_dt(op[1])
        elif kind == "reset":
            sim.reset_counters()
        elif kind == "update":
            sim.update_timestep()
        elif kind == "set_time":
            sim.set_time(sim.time() + op[1])
        elif kind == "upload":                                 # a changed state written back whole: the wet cells of a patch rise
            cur = sim.download()
            ys, xs = slice(rows // 3, rows // 3 + 3), slice(cols // 4, cols // 4 + 9)
            patch = cur[ys, xs]
            wet = (patch[..., 0] - sim.bed[ys, xs] > 1e-3) & live[ys, xs]
            patch[..., 0][wet] += real(op[1])
            patch[..., 1][wet] = np.maximum(patch[..., 1][wet], patch[..., 0][wet])
            sim.upload(cur)
            sim.update_timestep()                              # as the reference does after any write of the states
        elif kind == "rows2":                                  # two rows of the current buffer rise by a centimetre
            y0 = op[1]
            patch = sim.download()[y0:y0 + 2].copy()
            xs = slice(1, cols - 1) if op[2] else slice(0, cols)
            patch[:, xs, 0] += real(0.01) * live[y0:y0 + 2, xs]
            sim.upload_rows(patch, y0)
        elif kind == "blocks":                                 # the whole grid again, block by block (the wet cells a little higher)
            cur = sim.download()
            wet = (cur[..., 0] - sim.bed > 1e-3) & live
            wet[0, :] = wet[-1, :] = False; wet[:, 0] = wet[:, -1] = False
            cur[..., 0][wet] += real(op[2])
            cur[..., 1][wet] = np.maximum(cur[..., 1][wet], cur[..., 0][wet])
            y = 0
            for h in op[1]:
                sim.upload_rows(cur[y:y + h], y); y += h
        elif kind == "bed":                                    # the ground gives way a little under a patch (the water on it gets deeper)
            new_b = sim.bed.copy()
            ys, xs = slice(rows // 2, rows // 2 + 2), slice(max(1, cols // 3), min(cols - 1, cols // 3 + 7))
            ground = (new_b[ys, xs] > -9000) & (new_b[ys, xs] < 9000)
            new_b[ys, xs] -= (real(op[1]) * ground).astype(new_b.dtype)
            sim.upload(bed=new_b)
            sim.update_timestep()
        elif kind == "manning":                                # a new roughness map (uniform -> varying, or the other way round)
            new_n = (0.02 + op[1] * np.random.default_rng(int(op[1] * 1e6)).random((rows, cols))).astype(real) if manning_uniform else \
                np.full((rows, cols), 0.02 + op[1], real)
            manning_uniform = not manning_uniform
            sim.upload(manning=new_n)
        elif kind == "uniform":
            sim.add_uniform(op[1], op[2], op[3], op[4])
        elif kind == "gridded":
            sim.add_gridded(op[1], op[2], op[3], 0.0, 0.0, op[4])
        elif kind == "cell":
            sim.add_cell(op[1], op[2], op[3], op[4], op[5], op[6])
        elif kind == "clear":
            sim.clear_boundaries()
        elif kind == "save":
            sim.save()
        elif kind == "restore":
            sim.restore()
        elif kind == "sample":
            sim.sample()
        elif kind == "download":
            points.append(sim.download() if point is None else point(sim))
        elif extra is None or not extra(op, sim):
            raise ValueError(kind)
    finite = all(bool(np.isfinite((p if point is None else p[0])[live]).all()) for p in points)
    return dict(points=points, scalars=sim.scalars(), finite=finite, bed=sim.bed)


def run_on_oracle(seq):
    """The linearised sequence on the oracle (module docstring); `execute`'s dictionary."""
    assert seq["oracle_ok"], "the sequence holds a call the oracle does not have"
    twin = OracleTwin(seq["cfg"])
    out = execute(seq, twin)
    out["rebuilds"] = twin.rebuilds
    twin.close()
    return out


REFERENCE_ERROR_SHARE = 0.1                             # of FAST's bar: what the oracle's own rounding may take of it (reference_error)


def reference_error(seq, run=None):
    """The oracle's own error on an fp32 sequence: depth RMSE (m) of its final state against the same oracle computing in fp64 from
    the same (fp32-valued) inputs; 0 for an fp64 sequence, which has nothing more exact to be measured with.  The schemes branch
    (wet / dry, the HLLC wave pattern, the wall ring), so on some sequences fp32 rounding alone moves the oracle by far more than
    FAST's fp32 bar of 1e-4 m -- a dam break against the wall ring by 5e-2 m in 15 iterations, rain films on a slope by 2e-4 m in 35.
    There the fp32 oracle is no measure of an fp32 run at that bar: a FAST run rounds differently (its divisions, its fp64 time) and
    can only be expected to agree with the oracle as far as the oracle agrees with exact arithmetic.  test_gpu_host_calls.py holds an
    fp32 run to the oracle where this figure is below REFERENCE_ERROR_SHARE of the bar, which leaves nine tenths of it to the run."""
    cfg = seq["cfg"]
    if cfg["precision"] == "f64":
        return 0.0
    run = run or run_on_oracle(seq)
    wide = dict(cfg, precision="f64", st=cfg["st"].astype(np.float64), bed=cfg["bed"].astype(np.float64), man=cfg["man"].astype(np.float64))
    exact = run_on_oracle(dict(seq, cfg=wide))
    if not (run["finite"] and exact["finite"]):
        return float("inf")
    return depth_rmse(run["points"][-1], exact["points"][-1], run["bed"])


def digest(result):
    """What a run is held to, as one string: a SHA-256 of every comparison point, then the scalars."""
    return " ".join(hashlib.sha256(np.ascontiguousarray(p).tobytes()).hexdigest()[:24] for p in result["points"]) + " | " + \
        " ".join(repr(float(v)) if isinstance(v, float) else str(int(v)) for v in result["scalars"])


def describe(seq):
    c = seq["cfg"]
    return (f"{c['leg']} scheme {c['scheme']} {c['precision']} {c['cols']}x{c['rows']} {c['terrain']} dx {c['dx']}"
            f"{'' if c['dynamic'] else ' fixed-dt'}{' observers' if c['observers'] else ''}: " + " ".join(
                op_name(o) + (f"({o[1]})" if o[0] in ("batch", "split") else "") for o in seq["ops"]))


def depth_rmse(state_a, state_b, bed):
    """Depth RMSE (m) over every cell, the output derivation of the reference (depth = max(0, Z - bed))."""
    bed = bed.astype(np.float64)
    da = np.maximum(0.0, state_a[..., 0].astype(np.float64) - bed)
    db = np.maximum(0.0, state_b[..., 0].astype(np.float64) - bed)
    return float(np.sqrt(np.mean((da - db) ** 2)))
