"""Host-call sequences with the two actors that change the grid between the flux kernels -- the moving bed (hp_bed_shape_add /
hp_bed_apply, csrc/hp_bed.hpp) and link groups (hp_boundary_add_links, csrc/hp_links.hpp) -- and the stepwise twin they are held to
(shared by host_calls_actors_worker.py, test_gpu_host_calls_actors.py and test_host_calls_actors_cpu.py).

`make_actor_sequence(seed, leg)` takes host_calls.make_sequence(seed, leg) as it is and inserts up to MAX_EXTRA operations drawn from a
second generator (default_rng([seed, 1])): `shape`, `bed_apply`, `shapes_clear`, `links`, `links_read` and -- in every leg, because
the twin below can drop its boundary list -- `clear`.  A MUSCL-Hancock draw becomes Godunov or inertial (links are inert under
MUSCL-Hancock and the bed under it keeps its fixed-scene test); every other draw keeps its scheme, and with it its initial state.

The stepwise twin.  oracle.OracleSim.run has no place to apply links inside an iteration, so `StepTwin` steps the oracle's exported
grid functions itself, in the order orc_sim_run runs them (tests/test_links.py: StepLoop): boundaries on the source buffer in the
order added, orc_godunov_step / orc_inertial_step, orc_cfl_max_speed of the PRIMARY buffer (quirk Q1; 0 with a fixed timestep),
orc_advance, the flip.  Being Python it does not replay at a restore: it restates the checkpoint contract of include/hipims_mi.h
(the comment above hp_state_save) directly -- both buffers, the scalars and the ping-pong phase come back; the bed at the listed
cells comes back if no shape was added or cleared since the save, otherwise the bed stays and one warning is expected; the links'
records come back if no group was added or cleared since the save, otherwise they start from zero and one warning is expected; the
bed elsewhere, the Manning map and the boundary list are not rolled back.  test_host_calls_actors_cpu.py holds this restatement to
host_calls.OracleTwin's replay on every sequence of the old legs that is not MUSCL-Hancock.
A `bed_apply` on the twin is the round trip the contract names: frontend.BedShapes.apply on the current state and bed at the
twin's time, upload of the bed, upload of the state (which writes both buffers).  A link group is frontend.Links.apply on the
source buffer at its place in the boundary order.

What the twin cannot do: `rows2`, `blocks` (a partial upload) and `set_time`, as the oracle; a sequence with one of them has
`twin_ok == False` and is held to the engine's own run with pairs off alone.
"""
import ctypes as C
import hashlib

import numpy as np

import host_calls as hc
from host_calls import GODUNOV, INERTIAL, MUSCL, SPEC_MIN

LEGS = hc.LEGS
SEEDS_PER_LEG, CHUNK = 60, 30
# first seed of each leg: chosen so that the twin's own run stays finite on at least 95 % of the 60 seeds and every pattern the leg can
# produce occurs (test_host_calls_actors_cpu.py)
SEED_BASE = {"strict": 21100, "spec": 23400, "fast": 25200}
MAX_EXTRA = 6
APPLY_BATCHES = (1, 2, 3, 7, 8, 9)
TWIN_LESS = ("rows2", "blocks", "set_time")
ACTOR_KINDS = ("shape", "bed_apply", "shapes_clear", "links", "links_read")
PATTERNS = ("apply_between_pair_batches", "apply_behind_speculative_batch", "links_behind_speculative_batch", "pairs_after_links_cleared",
            "links_between_area_boundaries", "restore_across_apply", "restore_across_shape_change", "restore_across_links_change",
            "links_after_rows_upload")
LEG_PATTERNS = {leg: tuple(p for p in PATTERNS if ("speculative" not in p or leg == "spec") and (p != "links_after_rows_upload" or leg == "fast"))
                for leg in LEGS}
WEIR, ORIFICE, PUMP = 0, 1, 2


# ---- the sequences ---------------------------------------------------------------------------------------------------------------------
def bed_patch(rows, cols):
    """The cells host_calls.execute's `bed` operation lowers: no shape lists one of them, so "the bed at the listed cells" is what
    the shapes made it."""
    patch = np.zeros((rows, cols), bool)
    patch[rows // 2:rows // 2 + 2, max(1, cols // 3):min(cols - 1, cols // 3 + 7)] = True
    return patch


def make_actor_sequence(seed, leg="fast"):
    """host_calls.make_sequence(seed, leg) with the actors' operations inserted -- a pure function of (seed, leg)."""
    seq = hc.make_sequence(seed, leg)
    syn = hc._synthetic()
    rng = np.random.default_rng([seed, 1])
    cfg = dict(seq["cfg"])
    rows, cols, dx, real = cfg["rows"], cfg["cols"], cfg["dx"], cfg["st"].dtype.type
    if cfg["scheme"] == MUSCL:                               # re-drawn: Godunov or inertial
        cfg["scheme"] = GODUNOV if rng.random() < 0.75 else INERTIAL
        if cfg["scheme"] == INERTIAL:                        # (make_sequence's gentler start for that scheme)
            cfg["st"] = cfg["st"].copy()
            cfg["st"][..., 2:] *= real(0.1)
            if cfg["terrain"] == "dam":
                cfg["st"], cfg["bed"], cfg["man"] = syn.s_dam(cols, rows, dtype=real, levels=(1.2, 1.0))
    st, bed = cfg["st"], cfg["bed"]
    ops = list(seq["ops"])
    last = len(ops) - 1                                      # (the final download stays last)
    iterations = seq["iterations"]
    # the time the run covers, roughly: Courant 0.5 over sqrt(g h) of the deepest water, the first iterations shorter
    depth = float(np.max(np.where((st[..., 1] > -9000) & (bed < 9000), st[..., 0] - bed, 0.0)))
    per_iteration = 0.3 * dx / np.sqrt(9.81 * max(depth, 0.05)) if cfg["dynamic"] else cfg["fixed_dt"]
    span = max(iterations, 10) * per_iteration

    interior = np.zeros((rows, cols), bool)
    interior[1:-1, 1:-1] = True
    null = interior & (st[..., 1] <= -9000)
    shape_free = interior & ~bed_patch(rows, cols)           # cells no shape lists yet (over the whole sequence: a cleared cell is not listed again)
    link_free = interior.copy()                              # cells that are no link's end yet (over the whole sequence)

    def draw_shape():
        h, w = int(rng.integers(1, 6)), int(rng.integers(1, 9))
        y0, x0 = int(rng.integers(1, max(2, rows - 1))), int(rng.integers(1, max(2, cols - 1)))
        block = np.zeros((rows, cols), bool)
        block[y0:y0 + h, x0:x0 + w] = True
        if null.any() and rng.random() < 0.3:                # a null cell now and then
            ys, xs = np.nonzero(null)
            k = int(rng.integers(0, len(ys)))
            block[ys[k], xs[k]] = True
        cells = np.flatnonzero(block & shape_free)
        if cells.size == 0:
            cells = np.flatnonzero(shape_free)[:1]
        if cells.size == 0:
            return None
        cells = rng.permutation(cells)[:40]
        shape_free.reshape(-1)[cells] = False
        move = float(rng.uniform(-0.5, 0.5))                 # (small moves keep the runs finite)
        base = bed.reshape(-1)[cells].astype(np.float64)
        target = np.where(np.abs(base) < 9000.0, base + move, move)
        knots = int(rng.integers(2, 5))
        t0, t1 = sorted(rng.uniform(0.02, 0.95, 2) * span)
        times = np.linspace(t0, max(t1, t0 + 1e-3 * span), knots)
        fractions = rng.uniform(0.0, 1.0, knots)
        if rng.random() < 0.5:
            fractions[0] = 0.0
        if rng.random() < 0.5:
            fractions[-1] = 1.0
        return ("shape", cells.astype(np.uint64), target, np.stack([times, fractions], 1))

    def draw_links():
        n = int(rng.integers(1, 7))
        links = []
        for _ in range(n):
            free = np.flatnonzero(link_free)
            if free.size < 2:
                break
            a, b = (int(v) for v in rng.choice(free, 2, replace=False))
            free_null = np.flatnonzero(link_free & null)
            if free_null.size and rng.random() < 0.15:       # an end on a null cell now and then
                a = int(rng.choice(free_null))
                if a == b:
                    continue
            link_free.reshape(-1)[[a, b]] = False
            za, zb = float(st.reshape(-1, 4)[a, 0]), float(st.reshape(-1, 4)[b, 0])
            kind = int(rng.integers(0, 3))
            deep = cfg["terrain"] == "rough" and rng.random() < 0.25
            level = (min(za, zb) - 0.2) if deep else (max(za, zb) - float(rng.uniform(0.05, 0.5)))
            if kind == PUMP:
                level = za - float(rng.uniform(0.05, 0.5))
            size = 0.0 if rng.random() < 0.1 else float(rng.uniform(0.2, 1.5) * dx if kind == WEIR else rng.uniform(0.05, 0.3) * dx)
            limit = float(rng.uniform(0.0, 0.9)) if kind == WEIR else (np.inf if rng.random() < 0.4 else float(rng.uniform(0.05, 1.0) * dx))
            links.append(dict(a=a, b=b, kind=kind, one_way=int(rng.random() < 0.25), level=round(level, 4), size=size,
                              coeff=1.7 if kind == WEIR else 0.6, limit=limit))
        return ("links", links) if links else None

    # what to insert: a shape and an apply always, the rest by chance, at most MAX_EXTRA
    groups = int(rng.choice([0, 1, 1, 2, 2, 3]))
    wanted = ["shape", "bed_apply"] + ["links"] * groups
    optional = []
    if rng.random() < 0.6:
        optional.append("bed_apply")
    if groups and rng.random() < 0.7:
        optional.append("links_read")
    if rng.random() < (0.5 if groups else 0.1):
        optional.append("clear")
    if rng.random() < 0.25:
        optional.append("shapes_clear")
    if rng.random() < 0.2:
        optional.append("shape")
    wanted += [str(k) for k in rng.permutation(optional)][:MAX_EXTRA - len(wanted)]

    is_batch = lambda i, sizes=None: ops[i][0] == "batch" and (sizes is None or ops[i][1] in sizes)
    is_area = lambda i: ops[i][0] in ("uniform", "gridded")
    keys = []                                                # (key, order, kind): an extra with key i + 0.5 goes behind ops[i]
    for order, kind in enumerate(wanted):
        key = float(rng.integers(0, last)) - 0.5             # anywhere in front of the final download
        if kind == "bed_apply":                              # often straight after a batch of 1, 2, 3, 7, 8 or 9, and in front of another batch
            pair_sizes = [n for n in hc.BATCHES if n >= 2 and (leg != "spec" or n < SPEC_MIN)]      # (a speculative batch runs no pairs)
            between = [i for i in range(last - 1) if is_batch(i, APPLY_BATCHES) and is_batch(i, pair_sizes) and is_batch(i + 1, pair_sizes)]
            behind = [i for i in range(last) if is_batch(i, APPLY_BATCHES)]
            pick = between if between and rng.random() < 0.6 else behind if behind and rng.random() < 0.6 else None
            if pick:
                key = int(rng.choice(pick)) + 0.5
        elif kind == "links":
            amid = [i for i in range(last - 1) if is_area(i) and any(is_area(j) for j in range(i + 1, last))]
            long_batches = [i for i in range(last) if ops[i][0] == "batch" and ops[i][1] >= SPEC_MIN]
            r = float(rng.random())
            if amid and r < 0.4:                             # between two area boundaries: bdy_area's flush order
                key = int(rng.choice(amid)) + 0.5
            elif long_batches and r < 0.6:                   # straight behind a batch that may have been speculative
                key = int(rng.choice(long_batches)) + 0.5
        keys.append([key, order, kind])
    # a shape goes in front of the first apply
    first_shape = min((k for k in keys if k[2] == "shape"), key=lambda k: k[0])
    first_apply = min((k for k in keys if k[2] == "bed_apply"), key=lambda k: k[0])
    if first_shape[0] >= first_apply[0]:
        first_shape[0] = first_apply[0] - 0.25
    merged = sorted([(float(i), -1, op) for i, op in enumerate(ops)] + [(k, o, kind) for k, o, kind in keys], key=lambda e: (e[0], e[1]))
    out = []
    for _, order, op in merged:
        if order < 0:
            out.append(op)
        elif op == "shape":
            s = draw_shape()
            if s is not None:
                out.append(s)
        elif op == "links":
            l = draw_links()
            if l is not None:
                out.append(l)
        else:
            out.append((op,))
    new = dict(cfg=cfg, ops=out, iterations=iterations, oracle_ok=False, twin_ok=not any(o[0] in TWIN_LESS for o in out),
               patterns_old=seq["patterns"])
    new["patterns"] = count_patterns(new)
    return new


def count_patterns(seq):
    """How often the call patterns the actors' fuzz is about occur, from the operations alone (no run needed)."""
    cfg, found = seq["cfg"], dict.fromkeys(PATTERNS, 0)
    leg = cfg["leg"]
    pairs_cfg = cfg["scheme"] == GODUNOV and cfg["dynamic"]
    order = []                                               # the boundary list: "area" | "cell" | "links"
    shapes = 0
    saved = None                                             # since the save: dict(apply, shape, links)
    rows_pending = False
    cleared_links = False                                    # the last `clear` took a link group away and none was added since
    apply_state = 0                                          # 1: a pair batch ran last; 2: ... and a bed_apply behind it
    last_spec = False                                        # the last operation was a batch that may have run speculatively

    def pair_batch(n):
        if not pairs_cfg or "links" in order or n < 2:
            return False
        if leg == "fast":
            return "cell" not in order
        return not order and (leg == "strict" or n < SPEC_MIN)

    def spec_batch(n):
        fused = cfg["scheme"] == GODUNOV and "area" in order and "cell" not in order and "links" not in order
        return leg == "spec" and cfg["scheme"] == GODUNOV and n >= SPEC_MIN and "links" not in order and not fused

    for op in seq["ops"]:
        kind = op[0]
        passive = kind in ("download", "sample", "links_read")
        if kind in ("uniform", "gridded"):
            order.append("area")
        elif kind == "cell":
            order.append("cell")
        elif kind == "links":
            found["links_behind_speculative_batch"] += int(last_spec)
            order.append("links")
            cleared_links = False
            if saved is not None:
                saved["links"] = True
        elif kind == "clear":
            if "links" in order:
                cleared_links = True
                if saved is not None:
                    saved["links"] = True
            order = []
        elif kind == "shape":
            shapes += 1
            if saved is not None:
                saved["shape"] = True
        elif kind == "shapes_clear":
            if shapes and saved is not None:
                saved["shape"] = True
            shapes = 0
        elif kind == "bed_apply" and shapes:
            found["apply_behind_speculative_batch"] += int(last_spec)
            if saved is not None:
                saved["apply"] = True
            rows_pending = False
        elif kind == "save":
            saved = dict(apply=False, shape=False, links=False)
        elif kind == "restore":
            found["restore_across_apply"] += int(saved["apply"])
            found["restore_across_shape_change"] += int(saved["shape"])
            found["restore_across_links_change"] += int(saved["links"])
            saved = dict(apply=False, shape=False, links=False)
            rows_pending = False
        elif kind in ("rows2", "blocks"):
            rows_pending = True
        elif kind == "upload":
            rows_pending = False
        if kind in ("batch", "split"):
            n = op[1] if kind == "batch" else 1
            if "links" in order:
                i = order.index("links")
                found["links_between_area_boundaries"] += int("area" in order[:i] and "area" in order[i + 1:])
                found["links_after_rows_upload"] += int(rows_pending and leg == "fast")
            rows_pending = False
            pairs = kind == "batch" and pair_batch(n)
            if pairs and cleared_links:
                found["pairs_after_links_cleared"] += 1
                cleared_links = False
            if pairs and apply_state == 2:
                found["apply_between_pair_batches"] += 1
            apply_state = 1 if pairs else 0
            last_spec = kind == "batch" and spec_batch(n)
        elif kind == "bed_apply" and shapes:
            apply_state = 2 if apply_state in (1, 2) else 0
            last_spec = False
        elif not passive:
            apply_state = 0
            last_spec = False
    return found


def describe(seq):
    c = seq["cfg"]
    words = []
    for o in seq["ops"]:
        name = hc.op_name(o)
        words.append(name + (f"({o[1]})" if o[0] in ("batch", "split") else f"[{len(o[1])}]" if o[0] in ("shape", "links") else ""))
    return (f"{c['leg']} scheme {c['scheme']} {c['precision']} {c['cols']}x{c['rows']} {c['terrain']} dx {c['dx']}"
            f"{'' if c['dynamic'] else ' fixed-dt'}{' observers' if c['observers'] else ''}: " + " ".join(words))


# ---- the two things an actor sequence runs on ---------------------------------------------------------------------------------------
class ActorEngineSim(hc.EngineSim):
    """The HIP engine with the actors' calls.  `warnings`: a callable that counts the log sink's hp_state_restore warnings."""

    def __init__(self, cfg, warnings=lambda: 0):
        super().__init__(cfg)
        self.count_warnings, self.warnings_before = warnings, warnings()
        self.pairs_with_links = 0                            # pairs counted by batches that ran with a link group attached (must stay 0)
        self.links_active = 0

    @property
    def bed(self):                                           # (the bed as the device holds it: an apply moves it)
        return self.dom.download(self.hp.ARRAY_BED)

    @bed.setter
    def bed(self, value):
        pass

    def step_batch(self, n):
        super().step_batch(n)
        if self.dom.links_info()["groups"]:
            self.pairs_with_links += self.pairs_by_batch[-1]

    def bed_shape_add(self, cells, target, series): self.dom.bed_shape_add(cells, target, series)
    def bed_apply(self): self.dom.bed_apply()
    def add_links(self, links): self.dom.add_links(links)
    def download_bed(self): return self.dom.download(self.hp.ARRAY_BED)

    def bed_shapes_clear(self):                              # (hp_bed_info starts over with the shapes: keep what it counted)
        self.bed_counted = self.bed_totals()
        self.dom.bed_shapes_clear()

    def bed_totals(self):
        """(applies, cells changed) over the whole run, from hp_bed_info."""
        info, kept = self.dom.bed_info(), getattr(self, "bed_counted", (0, 0))
        return kept[0] + info["applies"], kept[1] + info["changed_total"]

    def links_records(self):
        rec = self.dom.links_read() if self.dom.links_info()["links"] else np.zeros(0, self.hp.LINK_RECORD_DTYPE)
        self.links_active = max(self.links_active, int(rec["active"].sum()))
        return rec

    def warnings(self):
        return self.count_warnings() - self.warnings_before


class StepTwin:
    """The oracle's grid functions stepped from Python, with the actors and the checkpoint contract restated (module docstring)."""

    def __init__(self, cfg):
        import oracle
        from hipims_mi import frontend
        if cfg["scheme"] == MUSCL:
            raise NotImplementedError("the stepwise twin runs Godunov and inertial only")
        self.cfg, self.frontend = cfg, frontend
        self.rows, self.cols = cfg["rows"], cfg["cols"]
        sim = oracle.OracleSim(cfg["cols"], cfg["rows"], dx=cfg["dx"], scheme=cfg["scheme"], precision=cfg["precision"], quirks=hc.QUIRKS_REFERENCE,
                               friction=cfg["friction"], dynamic_dt=cfg["dynamic"], fixed_dt=cfg["fixed_dt"],
                               dt_initial=cfg["fixed_dt"] if not cfg["dynamic"] else 0.001)
        self.sim, self.lib, self.p, self.creal, self.real = sim, sim.lib, sim.p, sim.creal, sim.real        # (its parameter block and library)
        self.flux = self.lib.orc_inertial_step if cfg["scheme"] == INERTIAL else self.lib.orc_godunov_step
        self.primary = np.zeros((self.rows, self.cols, 4), self.real)
        self.alt = np.zeros((self.rows, self.cols, 4), self.real)
        self.bed = np.zeros((self.rows, self.cols), self.real)
        self.man = np.zeros((self.rows, self.cols), self.real)
        self.sc = sim.Scalars(t=0.0, dt=sim.dt_initial, t_hydro=0.0, t_sync=0.0, batch_dt=0.0, batch_ok=0, batch_skipped=0)
        self.use_alt = 0
        self.boundaries = []                                 # ("uniform" | "gridded" | "cell", arguments) | ("links", frontend.Links)
        self.shapes, self.shapes_epoch, self.links_epoch = frontend.BedShapes(self.rows, self.cols), 0, 0
        self.mark, self.warned = None, 0
        self.applies = self.changed_total = 0

    # -- arrays
    def upload(self, state=None, bed=None, manning=None):
        if bed is not None:
            self.bed = np.array(bed, self.real)
        if manning is not None:
            self.man = np.array(manning, self.real)
        if state is not None:                                # both buffers, and the ping-pong phase starts over (orc_sim_upload)
            self.primary, self.alt, self.use_alt = np.array(state, self.real), np.array(state, self.real), 0

    def download(self): return (self.alt if self.use_alt else self.primary).copy()
    def download_bed(self): return self.bed.copy()
    def observers(self): pass
    def sample(self): pass
    def close(self): self.sim = None

    # -- time control
    def time(self): return self.sc.t
    def set_target(self, t): self.sc.t_sync = t
    def force_dt(self, dt): self.sc.dt = dt
    def reset_counters(self): self.sc.batch_dt, self.sc.batch_ok, self.sc.batch_skipped = 0.0, 0, 0
    def scalars(self): return (self.sc.t, self.sc.dt, self.sc.t_hydro, self.sc.batch_ok, self.sc.batch_skipped)
    def set_time(self, t): raise NotImplementedError("the twin has no call that sets the time")
    def upload_rows(self, patch, row0): raise NotImplementedError("the twin has no partial upload")

    def max_speed(self):
        if not self.cfg["dynamic"]:
            return 0.0
        return self.lib.orc_cfl_max_speed(C.byref(self.p), hc_ptr(self.primary), hc_ptr(self.bed))

    def update_timestep(self):
        self.lib.orc_update_timestep(C.byref(self.p), C.byref(self.sc), self.creal(self.max_speed()))

    # -- boundaries
    def add_uniform(self, definition, series, interval, length):
        self.boundaries.append(("uniform", (int(definition), np.ascontiguousarray(series, self.real), interval, length)))

    def add_gridded(self, definition, grids, resolution, off_x, off_y, interval):
        self.boundaries.append(("gridded", (int(definition), np.ascontiguousarray(grids, self.real), resolution, off_x, off_y, interval)))

    def add_cell(self, depth_def, discharge_def, cells, series, interval, length):
        self.boundaries.append(("cell", (int(depth_def), int(discharge_def), np.ascontiguousarray(cells, np.uint64),
                                         np.ascontiguousarray(series, self.real), interval, length)))

    def add_links(self, links):
        taken = [c for kind, b in self.boundaries if kind == "links" for c in np.concatenate([b.a, b.b])]
        L = self.frontend.Links(self.rows, self.cols, self.cfg["dx"], links)
        assert not set(taken) & set(np.concatenate([L.a, L.b]).tolist()), "a cell is an end of two links"
        self.boundaries.append(("links", L))
        self.links_epoch += 1

    def link_groups(self): return [b for kind, b in self.boundaries if kind == "links"]

    def links_records(self):
        import hipims_mi as hp
        groups = self.link_groups()
        return np.concatenate([L.records() for L in groups]) if groups else np.zeros(0, hp.LINK_RECORD_DTYPE)

    def clear_boundaries(self):
        if self.link_groups():
            self.links_epoch += 1
        self.boundaries = []

    # -- the moving bed
    def bed_shape_add(self, cells, target, series):
        self.shapes.add(cells, target, series, bed=self.bed)
        self.shapes_epoch += 1

    def bed_shapes_clear(self):
        if self.shapes.shapes:
            self.shapes, self.shapes_epoch = self.frontend.BedShapes(self.rows, self.cols), self.shapes_epoch + 1

    def bed_apply(self):
        if not self.shapes.shapes:                           # (HP_OK, nothing is enqueued)
            return
        state, bed = self.download(), self.bed.copy()
        self.changed_total += self.shapes.apply(state, bed, float(self.sc.t))
        self.applies += 1
        self.upload(bed=bed)
        self.upload(state=state)

    # -- iterations
    def step_batch(self, n):
        lib, p, r, ptr, sc = self.lib, C.byref(self.p), self.creal, hc_ptr, self.sc
        for _ in range(n):
            src, dst = (self.alt, self.primary) if self.use_alt else (self.primary, self.alt)
            for kind, b in self.boundaries:
                if kind == "uniform":
                    lib.orc_bdy_uniform(p, C.byref(sc), b[0], ptr(b[1]), C.c_uint(len(b[1])), r(b[2]), r(b[3]), ptr(src), ptr(self.bed), C.c_int(1))
                elif kind == "gridded":
                    g = b[1]
                    lib.orc_bdy_gridded(p, C.byref(sc), b[0], ptr(g), C.c_ulong(g.shape[0]), C.c_ulong(g.shape[1]), C.c_ulong(g.shape[2]), r(b[2]),
                                        r(b[3]), r(b[4]), r(b[5]), ptr(src), ptr(self.bed), C.c_int(1))
                elif kind == "cell":
                    lib.orc_bdy_cell(p, C.byref(sc), b[0], b[1], ptr(b[2]), C.c_ulong(len(b[2])), ptr(b[3]), C.c_ulong(len(b[3])), r(b[4]), r(b[5]),
                                     ptr(src), ptr(self.bed))
                else:
                    b.apply(src, self.bed, sc.dt)
            self.flux(p, r(sc.dt), ptr(self.bed), ptr(src), ptr(dst), ptr(self.man))
            lib.orc_advance(p, C.byref(sc), r(self.max_speed()))
            self.use_alt ^= 1

    def split(self): self.step_batch(1)

    # -- the checkpoint, as the header states it
    def save(self):
        listed = np.concatenate([s[0] for s in self.shapes.shapes]) if self.shapes.shapes else np.zeros(0, np.int64)
        self.mark = dict(primary=self.primary.copy(), alt=self.alt.copy(), use_alt=self.use_alt,
                         sc={k: getattr(self.sc, k) for k, _ in self.sc._fields_}, shapes_epoch=self.shapes_epoch, links_epoch=self.links_epoch,
                         listed=listed, bed_listed=self.bed.reshape(-1)[listed].copy(),
                         records=[(L.q_last.copy(), L.volume.copy(), L.active.copy()) for L in self.link_groups()])

    def restore(self):
        m = self.mark
        self.primary, self.alt, self.use_alt = m["primary"].copy(), m["alt"].copy(), m["use_alt"]
        for k, v in m["sc"].items():
            setattr(self.sc, k, v)
        if m["shapes_epoch"] != self.shapes_epoch:
            self.warned += 1                                 # "bed shapes were added or cleared after the state was saved: the bed is left as it is"
        elif len(m["listed"]):
            self.bed.reshape(-1)[m["listed"]] = m["bed_listed"]
        if m["links_epoch"] != self.links_epoch:
            self.warned += 1                                 # "link groups were added or cleared ...: the links' records start from zero"
            for L in self.link_groups():
                L.q_last, L.volume, L.active = np.zeros(len(L.links)), np.zeros(len(L.links)), np.zeros(len(L.links), np.uint64)
        else:
            for L, (q, v, a) in zip(self.link_groups(), m["records"]):
                L.q_last, L.volume, L.active = q.copy(), v.copy(), a.copy()

    def warnings(self): return self.warned


def hc_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- running -------------------------------------------------------------------------------------------------------------------------
def execute(seq, sim):
    """host_calls.execute with the actors' operations; a comparison point is (state, bed, the links' records), `reads` holds what
    every links_read saw and `warnings` the number of checkpoint warnings."""
    reads = []

    def extra(op, sim):
        kind = op[0]
        if kind == "shape":
            sim.bed_shape_add(op[1], op[2], op[3])
        elif kind == "bed_apply":
            sim.bed_apply()
        elif kind == "shapes_clear":
            sim.bed_shapes_clear()
        elif kind == "links":
            sim.add_links(op[1])
        elif kind == "links_read":
            reads.append(sim.links_records())
        else:
            return False
        return True

    out = hc.execute(seq, sim, extra=extra, point=lambda s: (s.download(), s.download_bed(), s.links_records()))
    out["reads"], out["warnings"] = reads, sim.warnings()
    return out


def run_on_twin(seq, cls=None):
    assert seq.get("twin_ok", seq["cfg"]["scheme"] != MUSCL), "the sequence holds a call the twin does not have"
    twin = (cls or StepTwin)(seq["cfg"])
    out = execute(seq, twin) if "twin_ok" in seq else hc.execute(seq, twin)
    out["applies"], out["changed_total"] = twin.applies, twin.changed_total
    out["links_active"] = int(sum(int(L.active.sum()) for L in twin.link_groups()))
    twin.close()
    return out


def wide(seq):
    """The same sequence in fp64 from the same (fp32-valued) inputs: what host_calls.reference_error measures an fp32 twin with."""
    cfg = seq["cfg"]
    return dict(seq, cfg=dict(cfg, precision="f64", st=cfg["st"].astype(np.float64), bed=cfg["bed"].astype(np.float64), man=cfg["man"].astype(np.float64)))


def reference_error(seq, run):
    """host_calls.reference_error's rule with the stepwise twin: the fp32 twin's depth RMSE (m) against itself in fp64; 0 in fp64."""
    if seq["cfg"]["precision"] == "f64":
        return 0.0
    exact = run_on_twin(wide(seq))
    if not (run["finite"] and exact["finite"]):
        return float("inf")
    return hc.depth_rmse(run["points"][-1][0], exact["points"][-1][0], run["bed"])


def digest(result):
    """What a run of an actor sequence is held to, as one string: state, bed and records at every download, the records at every
    links_read, the scalars, the checkpoint warnings."""
    h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]
    return " ".join(":".join(h(a) for a in p) for p in result["points"]) + " | " + " ".join(h(r) for r in result["reads"]) + " | " + \
        " ".join(repr(float(v)) if isinstance(v, float) else str(int(v)) for v in result["scalars"]) + f" | warnings {result['warnings']}"


# ---- two scenarios by hand (host_calls_actors_worker.py runs them on the engine, test_gpu_host_calls_actors.py on the twin) ------------
SCENARIOS = ("pairs_resume_after_links_cleared", "apply_behind_replayed_batches")
SCENARIO_RAIN = np.array([[0.0, 600.0], [0.7, 200.0], [1.4, 50.0], [2.1, 0.0]])
# through the step between the two pools of s_rough (0.75 m left of column 32, 0.35 m right of it): a weir, a culvert, a pump uphill
SCENARIO_LINKS = [dict(a=(10, 10), b=(50, 10), kind=WEIR, level=0.5, size=1.0, coeff=1.7, limit=0.5),
                  dict(a=(12, 20), b=(52, 22), kind=ORIFICE, level=0.2, size=0.3, coeff=0.6, limit=np.inf),
                  dict(a=(50, 30), b=(8, 30), kind=PUMP, level=0.0, size=0.2)]


def scenario_cfg(name):
    syn = hc._synthetic()
    if name == "pairs_resume_after_links_cleared":           # FAST fp64, 64 x 37 rough terrain under rain
        st, bed, man = syn.s_rough(64, 37, manning=None, seed=31)
        math = "fast"
    elif name == "apply_behind_replayed_batches":            # STRICT fp64, 65 x 37 with dry ground and null cells
        st, bed, man = hc.rough_with_nulls(65, 37)
        math = "strict"
    else:
        raise ValueError(name)
    return dict(seed=0, leg=math, scheme=GODUNOV, precision="f64", cols=st.shape[1], rows=st.shape[0], dx=1.0, terrain="rough", st=st, bed=bed, man=man,
                friction=True, dynamic=True, fixed_dt=0.001, observers=False, math=math)


def run_scenario(name, sim):
    """The scenario's calls on `sim` (ActorEngineSim or StepTwin): state, bed and scalars after every batch, the links' records."""
    cfg = sim.cfg
    cols = cfg["cols"]
    out = dict(states=[], beds=[], scalars=[], records=[])

    def batch(n):
        sim.step_batch(n)
        out["states"].append(sim.download()); out["beds"].append(sim.download_bed()); out["scalars"].append([float(v) for v in sim.scalars()])

    sim.upload(cfg["st"], cfg["bed"], cfg["man"])
    sim.set_target(1e9)
    if name == "pairs_resume_after_links_cleared":
        sim.add_uniform(hc.UNIFORM_RAIN, SCENARIO_RAIN, 0.7, 2.1)
        batch(8)
        sim.add_links(SCENARIO_LINKS)
        batch(7)
        out["records"].append(sim.links_records())
        sim.clear_boundaries()
        batch(8)
    else:
        # a breach that opens over the whole run (it is moving at both applies) through wet ground, a null cell (7, 5) and its
        # neighbours, and a barrier that rises on the dry hill side
        breach = np.array([y * cols + x for y in range(4, 8) for x in range(5, 10)], np.uint64)
        barrier = np.array([y * cols + x for y in range(18, 22) for x in range(38, 43)], np.uint64)
        sim.bed_shape_add(breach, cfg["bed"].reshape(-1)[breach.astype(np.int64)].astype(np.float64).clip(-9000, 9000) - 0.4, np.array([[0.0, 0.0], [20.0, 1.0]]))
        sim.bed_shape_add(barrier, 0.9, np.array([[0.0, 0.1], [0.5, 0.3], [30.0, 1.0]]))
        batch(9)
        sim.bed_apply()
        batch(5)
        sim.save()
        batch(9)
        sim.bed_apply()
        out["states"].append(sim.download()); out["beds"].append(sim.download_bed()); out["scalars"].append([float(v) for v in sim.scalars()])
        sim.restore()
        batch(9)
    out["warnings"] = sim.warnings()
    return out
