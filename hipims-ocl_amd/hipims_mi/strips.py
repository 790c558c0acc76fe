"""1-D row-strip decomposition of ONE logical grid over the GPUs of a node (one process per GPU).

Replaces the reference's overlapping-domain links (src/Domain/Links/CDomainLink.cpp:286-382: strips staged through
host memory, optionally MPI, several iterations between exchanges, forecast/rollback) with the `timestep` sync
semantic only (src/CModel.cpp:650-694): every iteration

    step_begin  : boundaries + flux kernel + LOCAL max wave speed          (device, domain stream)
    halo        : `g` ghost rows of the NEW state <-> the two strip neighbours   (RCCL send/recv over xGMI)
    all-reduce  : MAX of one scalar (the wave speed; replaces MPI_Allreduce(MIN dt), CMPIManager.cpp:852-861)
    step_end    : tst_Advance_Normal on every rank redundantly -> identical dt everywhere, no host round trip

so a decomposed run is bit-identical to the single-GPU run (max is exact and order independent).
g = 1 row for Godunov, 2 for MUSCL-Hancock (13-point stencil).

Overlap: with more than one rank the engine computes the row segments next to the ghost rows on a second stream
(hp_set_halo_overlap); the halo transfer is ordered after that stream only, so it travels while the interior
segments are still being computed on the domain's stream, which waits for it just before step_end.

The exchange is written against torch.distributed so that the very same code runs over RCCL ("nccl") on GPUs and
over "gloo" on CPU tensors in the world_size-2 tests (tests/test_strips_gloo.py, with the oracle as engine).
Rehearsal transport: `backend="gloo"` together with the HIP engine stages the ghost rows and the scalar through
host memory.  It exists so that the whole multi-rank path (partition, strip inputs, bench.py's N > 1 branch) can be
run with several processes on ONE GPU, where RCCL refuses to put two ranks; it is not a production path.
"""
from __future__ import annotations

import contextlib
import os

import numpy as np

from . import (KERNEL_AUTO, MATH_FAST, PTR_CFL_MAX, PTR_STATE_NEXT_SRC, PTR_STATE_OTHER, QUIRKS_REFERENCE,
               SCHEME_GODUNOV, SCHEME_INERTIAL, SCHEME_MUSCL_HANCOCK, Domain)
from . import synthetic as syn


FLUX_KERNELS = {SCHEME_GODUNOV: "hp::godunov_march", SCHEME_MUSCL_HANCOCK: "hp::muscl_march", SCHEME_INERTIAL: "hp::inertial_march"}


def ghost_rows(scheme) -> int:
    return 2 if scheme == SCHEME_MUSCL_HANCOCK else 1


def partition(global_rows: int, world: int, g: int):
    """Rows owned by each rank and the rows it stores: [(own_lo, own_hi, local_lo, local_hi)] (global indices).
    `g` = ghost rows stored per interior side (the stencil reach, or a multiple of it for several iterations per exchange)."""
    parts = []
    for k in range(world):
        own_lo, own_hi = (k * global_rows) // world, ((k + 1) * global_rows) // world
        parts.append((own_lo, own_hi, max(0, own_lo - g), min(global_rows, own_hi + g)))
    for own_lo, own_hi, _, _ in parts:
        if own_hi - own_lo < 2 * g + 1:
            raise ValueError("strip thinner than its halo")
    return parts


def assemble_outputs(parts):
    """The ranks' owned-row rasters ({name: array}, in rank order = south to north) as rasters of the whole grid."""
    return {name: np.concatenate([p[name] for p in parts], axis=0) for name in parts[0]}


def assemble_overviews(parts, aggregates):
    """[per rank: (first_block_row, [one overview per pair])] -> [one overview of the whole grid per pair]: the ranks' owned rows
    cover the grid, so the combined block rows start at 0 (frontend.combine_overviews: integer folds, equal to the single domain's
    overview in every bit wherever the strips are cut)."""
    from . import frontend
    out = []
    for k, aggregate in enumerate(aggregates):
        first, combined = frontend.combine_overviews([(f, arrays[k]) for f, arrays in parts], aggregate)
        assert first == 0, first
        out.append(combined)
    return out


def combine_stats(parts, local_los, cols):
    """Domain.stats() of every rank's OWNED rows (rank order) as the statistics of the whole grid: counts added and maxima
    combined exactly -- equal maxima go to the lowest cell id, i.e. to the first rank that has them --, volumes added in
    rank order.  Cell ids become global ones (y * cols + x): `local_los` are the global rows of the ranks' local row 0."""
    out = dict(cells=0, cells_wet=0, volume=0.0, max_depth=0.0, max_speed=0.0, max_depth_cell=None, max_speed_cell=None)
    for p, lo in zip(parts, local_los):
        out["cells"] += p["cells"]
        out["cells_wet"] += p["cells_wet"]
        out["volume"] += p["volume"]
        for val, cell in (("max_depth", "max_depth_cell"), ("max_speed", "max_speed_cell")):
            if p[cell] is not None and (out[cell] is None or p[val] > out[val]):
                out[val], out[cell] = p[val], p[cell] + lo * cols
    return out


def probe_points(gauges, sections):
    """The probe recorder over strips.  A section's sum has a fixed order (csrc/hp_probes.hpp), which sums per rank would change.
    So every POINT -- a gauge, or one cell of a section -- is recorded as a gauge by the rank that owns its row.
    -> (gauges[G, 2], [frontend.Section], points[G + sum(m), 2]): the gauges, then every section's cells, as (x, y)."""
    from . import frontend
    g = np.asarray(gauges, dtype=np.int64).reshape(-1, 2)
    secs = [frontend.Section(np.asarray(s[0], dtype=np.int64).reshape(-1, 2), np.asarray(s[1], np.int8).reshape(-1),
                             np.asarray(s[2], np.int8).reshape(-1)) for s in sections]
    points = np.concatenate([g] + [s.cells for s in secs], axis=0)
    if not len(points):
        raise ValueError("neither a gauge nor a section")
    return g, secs, points


def assemble_probes(parts, gauges, sections, dx):
    """`parts`: per rank (indices into probe_points' list, t[n], values[n, k, 4]) of the points it owns, or None.  The gauges'
    values are the ranks' own; a section's discharge is formed from its cells' values in the kernel's order
    (frontend.section_terms, fold_section_terms: an uncounted cell's depth is NODATA, i.e. not wet), so the result equals the
    single domain's record bit for bit.  -> {"t": [n], "gauges": [n, G, 4], "sections": [n, S]}"""
    from . import frontend
    parts = [p for p in parts if p is not None]
    t = np.array(parts[0][1])
    G = len(gauges)
    values = np.empty((len(t), G + sum(len(s.cells) for s in sections), 4))
    for idx, t_k, v in parts:
        if not np.array_equal(t_k, t):
            raise RuntimeError("the ranks' probe samples were taken at different model times")
        values[:, idx] = v
    q = np.empty((len(t), len(sections)))
    at = G
    for k, s in enumerate(sections):
        v = values[:, at:at + len(s.cells)]
        at += len(s.cells)
        for n in range(len(t)):
            q[n, k] = frontend.fold_section_terms(frontend.section_terms(s.wx, s.wy, v[n, :, 1], v[n, :, 2], v[n, :, 3]), dx)
    return dict(t=t, gauges=values[:, :G].copy(), sections=q)


def links_strip_verdict(row_a, row_b, local_lo, local_hi, stale_lo=0, stale_hi=0):
    """csrc/hp_links.hpp: links_strip_verdict.  0: the strip that stores the global rows [local_lo, local_hi) ignores the link
    between rows row_a and row_b, 2: it computes it, 1: it cannot run it -- it stores one end only, or one end on a row of its
    outermost reach of ghost rows (`stale_*` rows per side: valid on every second iteration only) and the other on a row that is
    always valid."""
    a_in, b_in = local_lo <= row_a < local_hi, local_lo <= row_b < local_hi
    if not a_in and not b_in:
        return 0
    if a_in != b_in:
        return 1
    a_stale = row_a < local_lo + stale_lo or row_a >= local_hi - stale_hi
    b_stale = row_b < local_lo + stale_lo or row_b >= local_hi - stale_hi
    return 2 if a_stale == b_stale else 1


def links_refused(links, cols, parts, reach):
    """The first (link, rank) whose verdict is 1 over the strips `parts` (partition's), or None.  `reach`: the scheme's stencil
    reach; a strip that stores more ghost rows than that holds the rest on every second iteration only."""
    rows = parts[-1][1]
    for k in range(len(links)):
        ya, yb = int(links["cell_a"][k]) // cols, int(links["cell_b"][k]) // cols
        for rank, (own_lo, own_hi, lo, hi) in enumerate(parts):
            stale_lo = max(0, (own_lo - lo) - reach) if lo > 0 else 0
            stale_hi = max(0, (hi - own_hi) - reach) if hi < rows else 0
            if links_strip_verdict(ya, yb, lo, hi, stale_lo, stale_hi) == 1:
                return k, rank
    return None


class HipEngine:
    """The HIP domain of one strip + zero-copy torch views of its device buffers."""

    def __init__(self, cols, local_rows, global_rows, row_offset, **kw):
        import torch
        self.flux_kernel_name = FLUX_KERNELS[kw.get("scheme", SCHEME_GODUNOV)]
        self.torch = torch
        self.domain = Domain(cols, local_rows, global_rows=global_rows, row_offset=row_offset, **kw)
        self.device = torch.device("cuda", kw.get("device", 0))
        torch.cuda.set_device(self.device)
        # run torch's collectives in order with the engine's kernels: make the domain's stream torch's current one
        self.stream = torch.cuda.ExternalStream(self.domain.stream_ptr(), device=self.device)
        self.halo_stream = torch.cuda.ExternalStream(self.domain.halo_stream_ptr(), device=self.device)
        torch.cuda.set_stream(self.stream)
        self._views = {}

    def set_halo_overlap(self, on):
        self.domain.set_halo_overlap(on)
        self._overlap = bool(on)

    def halo_context(self):
        """Stream context the halo send/recv is issued in: the collective library orders itself after the work of
        torch's current stream, which inside this context is the stream the halo segments were computed on."""
        if getattr(self, "_overlap", False):
            return self.torch.cuda.stream(self.halo_stream)
        return contextlib.nullcontext()

    def _view(self, which):
        ptr = self.domain.device_ptr(which)
        key = (which, ptr)
        if key not in self._views:
            self._views[key] = self.torch.as_tensor(self.domain.device_array(which), device=self.device)
        return self._views[key]

    def step_begin(self):
        self.domain.step_begin()

    def step_end(self):
        self.domain.step_end()

    def needs_reduction(self):
        return self.domain.step_needs_reduction()

    def new_state(self):
        """Buffer the iteration in flight has just written (valid between step_begin and step_end)."""
        return self._view(PTR_STATE_OTHER)

    def cfl_slot(self):
        return self._view(PTR_CFL_MAX)

    def upload(self, st, bed, man):
        self.domain.upload(st, bed, man)

    def download(self):
        return self.domain.download()

    def derive(self, values, dtype=np.float64, row0=0, nrows=None):
        return self.domain.derive(values, dtype=dtype, row0=row0, nrows=nrows)

    def overview(self, values, aggregates, factor, dtype=np.float64, row0=0, nrows=None):
        return self.domain.overview(values, aggregates, factor, dtype=dtype, row0=row0, nrows=nrows)

    def overview_shape(self, factor, row0=0, nrows=None):
        return self.domain.overview_shape(factor, row0=row0, nrows=nrows)

    def sparse(self, values, select="depth", above=0.0, dtype=np.float64, row0=0, nrows=None):
        return self.domain.sparse(values, select=select, above=above, dtype=dtype, row0=row0, nrows=nrows)

    def stats(self, row0=0, nrows=None):
        return self.domain.stats(row0=row0, nrows=nrows)

    # the moving bed (Domain.bed_*)
    def bed_shape_add(self, cells, target, series):
        self.domain.bed_shape_add(cells, target, series)

    def bed_shapes_clear(self):
        self.domain.bed_shapes_clear()

    def bed_apply(self):
        self.domain.bed_apply()

    def download_bed(self):
        from . import ARRAY_BED
        return self.domain.download(ARRAY_BED)

    # link groups (Domain.add_links)
    def add_links(self, links):
        self.domain.add_links(links)

    def links_read(self, first=0, count=None):
        return self.domain.links_read(first, count)

    # the open boundary (Domain.add_open)
    def add_open(self, segments):
        self.domain.add_open(segments)

    def open_read(self, first=0, count=None):
        return self.domain.open_read(first, count)

    # the infiltration (Domain.add_infiltration)
    def add_infiltration(self, soil, classes, initial=None):
        self.domain.add_infiltration(soil, classes, initial)

    def infiltration_read(self, row0=0, nrows=None):
        return self.domain.infiltration_read(row0, nrows)

    # the tracer (Domain.tracer_*)
    def tracer_enable(self, initial=None):
        self.domain.tracer_enable(initial)

    def tracer_disable(self):
        self.domain.tracer_disable()

    def tracer_add_source(self, cells, series):
        self.domain.tracer_add_source(cells, series)

    def tracer_read(self, row0=0, nrows=None):
        return self.domain.tracer_read(row0, nrows)

    def tracer_write(self, raster, row0=0):
        self.domain.tracer_write(raster, row0)

    def tracer_info(self):
        return self.domain.tracer_info()

    # the peak tracker (Domain.peaks_*)
    def peaks_enable(self, values, arrival_depth=0.01):
        self.domain.peaks_enable(values, arrival_depth=arrival_depth)

    def peaks_disable(self):
        self.domain.peaks_disable()

    def peaks_reset(self):
        self.domain.peaks_reset()

    def peaks_sample(self):
        self.domain.peaks_sample()

    def peaks(self, values=None, dtype=np.float64, row0=0, nrows=None):
        return self.domain.peaks(values, dtype=dtype, row0=row0, nrows=nrows)

    def peaks_info(self):
        return self.domain.peaks_info()

    # the probe recorder (Domain.probes_*)
    def probes_enable(self, gauges=(), sections=(), capacity=4096):
        self.domain.probes_enable(gauges, sections, capacity=capacity)

    def probes_disable(self):
        self.domain.probes_disable()

    def probes_sample(self):
        self.domain.probes_sample()

    def probes(self):
        return self.domain.probes()

    def probes_info(self):
        return self.domain.probes_info()

    # the zone recorder (Domain.zones_*)
    def zones_enable(self, ids, zone_count=None, flood_depth=0.1, capacity=4096):
        self.domain.zones_enable(ids, zone_count, flood_depth=flood_depth, capacity=capacity)

    def zones_disable(self):
        self.domain.zones_disable()

    def zones_reset(self):
        self.domain.zones_reset()

    def zones_sample(self):
        self.domain.zones_sample()

    def zone_records(self):
        return self.domain.zone_records()

    def zones(self):
        return self.domain.zones()

    def zones_info(self):
        return self.domain.zones_info()

    def set_target_time(self, t):
        self.domain.set_target_time(t)

    def scalars(self):
        s = self.domain.read_scalars()
        return dict(t=s["time"], dt=s["timestep"], batch_ok=s["batch_successful"], batch_skipped=s["batch_skipped"])

    def sync(self):
        self.domain.sync()

    def close(self):
        self.domain.close()


class SingleRunner:
    """N = 1: the plain batch call, no torch involved."""

    def __init__(self, cols, rows, **kw):
        self.domain = Domain(cols, rows, **kw)
        self.local_rows_total = rows
        self.local_lo, self.local_hi = 0, rows
        self.flux_kernel_name = FLUX_KERNELS[kw.get("scheme", SCHEME_GODUNOV)]

    def upload(self, st, bed, man):
        self.domain.upload(st, bed, man)

    def set_target_time(self, t):
        self.domain.set_target_time(t)

    def step(self, n):
        self.domain.step_batch(n)

    def save(self):
        self.domain.state_save()

    def restore(self):
        self.domain.state_restore()

    def barrier(self):
        self.domain.sync()

    def max_over_ranks(self, x):
        return x

    def close(self):
        self.domain.close()


class StripRunner:
    """One rank of the strip-decomposed run.  `engine_factory(cols, local_rows, global_rows, row_offset)` lets the
    CPU tests substitute an oracle-backed engine; the default builds the HIP engine."""

    def __init__(self, cols, rows, scheme=SCHEME_GODUNOV, precision="f64", rank=0, world=1, device=0,
                 engine_factory=None, backend=None, init_process_group=True, overlap=None, loop=None, exchange_period=None,
                 area_boundaries=False, **kw):
        import torch
        import torch.distributed as dist
        self.torch, self.dist = torch, dist
        self.cols, self.rows, self.rank, self.world = cols, rows, rank, world
        # ghost rows stored per interior side: one stencil reach, exchanged after every iteration -- or two, exchanged after
        # every second one by the library's own strip loop (the strip recomputes a reach of its neighbour's rows in between).
        # None = the best the configuration allows (round 6): two reaches wherever the strips can then run iteration PAIRS -- the HIP
        # engine under the library's own loop (one GPU per rank), Godunov scheme, FAST arithmetic, the tuned kernel, no area boundaries
        # to come (`area_boundaries`: the caller's word) -- whether every rank really can is settled by the ranks' handshake at the
        # start of each batch (hp_strip_step_batch); everything else exchanges after every iteration, as an explicit 1 does.
        if exchange_period is None:
            from . import KERNEL_AUTO, MATH_FAST
            want_loop = loop or os.environ.get("HIPIMS_MI_STRIP_LOOP", "cxx" if (engine_factory is None and (backend or "nccl") == "nccl") else "torch")
            pairs = (engine_factory is None and (backend or "nccl") == "nccl" and want_loop == "cxx" and world > 1 and scheme == SCHEME_GODUNOV
                     and kw.get("math_mode", MATH_FAST) == MATH_FAST and kw.get("kernel", KERNEL_AUTO) == KERNEL_AUTO and not area_boundaries
                     and os.environ.get("HP_TWO_STEP", "") != "0")
            if pairs:
                # (two reaches belong to the library's own loop: without the collective library -- every rank finds that out the same
                # way -- the run falls back to the torch loop below, which exchanges after every iteration)
                from . import HipimsError, comm_load
                try:
                    comm_load()
                except HipimsError:
                    pairs = False
            exchange_period = 2 if pairs else 1
        if exchange_period not in (1, 2):
            raise ValueError("exchange_period must be 1 or 2")
        self.exchange_period = exchange_period
        self.g = ghost_rows(scheme) * exchange_period
        self.scheme, self.precision = scheme, precision
        self.parts = partition(rows, world, self.g)
        self.own_lo, self.own_hi, self.local_lo, self.local_hi = self.parts[rank]
        self.local_rows_total = self.local_hi - self.local_lo
        if engine_factory is None:
            self.engine = HipEngine(cols, self.local_rows_total, rows, self.local_lo, scheme=scheme,
                                    precision=precision, device=device, ghost_rows=self.g if exchange_period > 1 else 0, **kw)
            backend = backend or "nccl"
        else:
            self.engine = engine_factory(cols, self.local_rows_total, rows, self.local_lo)
            backend = backend or "gloo"
        self.domain = getattr(self.engine, "domain", None)
        self.flux_kernel_name = getattr(self.engine, "flux_kernel_name", "")
        if init_process_group and not dist.is_initialized():
            kwargs = {}
            if backend == "nccl":
                kwargs["device_id"] = torch.device("cuda", device)
            dist.init_process_group(backend=backend, rank=rank, world_size=world, **kwargs)
        # who runs the per-iteration loop: "cxx" = the library itself over RCCL (hp_strip_step_batch: a handful of
        # enqueues per iteration, no Python in the loop), "torch" = this class over torch.distributed.  The C++ loop
        # needs RCCL, i.e. one GPU per rank; rehearsals on a shared GPU (gloo) and the CPU tests use the torch loop.
        if loop is None:
            loop = os.environ.get("HIPIMS_MI_STRIP_LOOP", "cxx" if (engine_factory is None and backend == "nccl") else "torch")
        self.loop = loop
        self.peer_max = 0          # what the ranks agreed on (C++ loop): 0 library, 1 mailboxes, 2 mailboxes + pushed ghost rows
        if exchange_period > 1 and loop != "cxx":
            raise ValueError("several iterations per exchange are the C++ strip loop's (loop='cxx')")
        if loop == "cxx":
            if engine_factory is not None or backend != "nccl":
                raise ValueError("the C++ strip loop runs on the HIP engine over RCCL only")
            from . import HipimsError, comm_load, comm_unique_id
            try:
                comm_load()
            except HipimsError as e:
                # every rank loads the same library the same way, so they all land here together: the run goes on with
                # the torch loop (slower host side, same results) and says so in `loop`
                if "HIPIMS_MI_STRIP_LOOP" in os.environ:
                    raise
                import sys
                if exchange_period > 1:
                    raise
                print(f"[hipims_mi] C++ strip loop unavailable ({e}); using the torch loop", file=sys.stderr, flush=True)
                self.loop = loop = "torch"
        if loop == "cxx":
            from . import comm_unique_id
            box = [comm_unique_id() if rank == 0 else None]
            if world > 1:
                dist.broadcast_object_list(box, src=0)        # the id travels by the host's own means (here: torch)
            self.domain.strip_comm_init(box[0], rank, world)
            # the maximum over the strips: peer-written mailboxes where every rank can reach every other one's (the
            # library tests that and the ranks agree), the collective library's all-reduce otherwise
            if world > 1 and os.environ.get("HIPIMS_MI_PEER_MAX", "1") != "0":
                tickets = [None] * world
                dist.all_gather_object(tickets, self.domain.strip_peer_ticket())
                self.peer_max = self.domain.strip_peer_connect(tickets, rank)
        self.south = rank - 1 if rank > 0 else None
        self.north = rank + 1 if rank < world - 1 else None
        self.staged = engine_factory is None and backend == "gloo"      # device buffers, host transport (rehearsal)
        self._halo_ops = {}
        if overlap is None:
            overlap = world > 1
        if hasattr(self.engine, "set_halo_overlap"):
            self.engine.set_halo_overlap(overlap)

    # ---- data placement ----
    def local_slice(self):
        return slice(self.local_lo, self.local_hi)

    def make_s_dam(self, real, levels=(10.0, 1.0)):
        """This rank's rows of the global S-DAM input (built strip by strip: a 16384 x 8192 fp64 state is 4 GiB)."""
        st, bed, man = syn.s_dam(self.cols, self.local_rows_total, dtype=real, levels=levels)
        # s_dam walls all four edges of what it builds; only the global south/north rows are walls
        z_col = st[1, :, 0].copy() if self.local_rows_total > 2 else None
        if self.local_lo > 0:
            st[0, :, 0] = z_col; st[0, :, 1] = z_col; bed[0, :] = 0.0
            st[0, 0, :] = 0; st[0, -1, :] = 0; bed[0, 0] = bed[0, -1] = syn.WALL_BED
        if self.local_hi < self.rows:
            st[-1, :, 0] = z_col; st[-1, :, 1] = z_col; bed[-1, :] = 0.0
            st[-1, 0, :] = 0; st[-1, -1, :] = 0; bed[-1, 0] = bed[-1, -1] = syn.WALL_BED
        return st, bed, man

    def upload(self, st_local, bed_local, man_local):
        self._bed_local = None if bed_local is None else np.array(bed_local)     # (the host-side probe recorder's bed)
        self.engine.upload(st_local, bed_local, man_local)

    def upload_global(self, st, bed, man):
        sl = self.local_slice()
        self.upload(st[sl], bed[sl], man[sl])

    def set_target_time(self, t):
        self.engine.set_target_time(t)

    # ---- the per-iteration protocol ----
    def _start_halo(self):
        """Queue the ghost-row exchange of the iteration in flight; returns the requests to wait for."""
        dist, g = self.dist, self.g
        new = self.engine.new_state()            # [local_rows, cols, 4]
        if self.staged:
            return self._start_halo_staged(new)
        ops = self._halo_ops.get(new.data_ptr())  # the two ping-pong buffers alternate: build each list once
        if ops is None:
            n = new.shape[0]
            ops = []
            if self.south is not None:
                ops.append(dist.P2POp(dist.isend, new[g:2 * g], self.south))          # my first owned rows
                ops.append(dist.P2POp(dist.irecv, new[0:g], self.south))              # into my south ghost rows
            if self.north is not None:
                ops.append(dist.P2POp(dist.isend, new[n - 2 * g:n - g], self.north))  # my last owned rows
                ops.append(dist.P2POp(dist.irecv, new[n - g:n], self.north))          # into my north ghost rows
            self._halo_ops[new.data_ptr()] = ops
        if not ops:
            return []
        ctx = self.engine.halo_context() if hasattr(self.engine, "halo_context") else contextlib.nullcontext()
        with ctx:
            return dist.batch_isend_irecv(ops)

    def _start_halo_staged(self, new):
        """Rehearsal transport: rows go device -> host -> gloo -> host -> device."""
        dist, g, n = self.dist, self.g, new.shape[0]
        ops, landings = [], []
        with self.engine.halo_context():                      # .cpu() waits for the halo segments only
            for peer, send, recv in ((self.south, new[g:2 * g], new[0:g]), (self.north, new[n - 2 * g:n - g], new[n - g:n])):
                if peer is None:
                    continue
                buf = self.torch.empty(recv.shape, dtype=recv.dtype)
                ops += [dist.P2POp(dist.isend, send.cpu(), peer), dist.P2POp(dist.irecv, buf, peer)]
                landings.append((recv, buf))
        reqs = dist.batch_isend_irecv(ops) if ops else []

        class _Landing:
            def wait(_self):
                for r in reqs:
                    r.wait()
                for recv, buf in landings:
                    recv.copy_(buf)                           # on the domain stream, before step_end
        return [_Landing()] if ops else []

    def _all_reduce_max(self, slot):
        if self.staged:
            host = slot.cpu()                                 # waits for the whole flux launch
            self.dist.all_reduce(host, op=self.dist.ReduceOp.MAX)
            slot.copy_(host)
        else:
            self.dist.all_reduce(slot, op=self.dist.ReduceOp.MAX)

    def _exchange_halo(self):
        for req in self._start_halo():
            req.wait()

    def step(self, n):
        if self.loop == "cxx":
            self.domain.strip_step_batch(n)
            return
        dist = self.dist
        for _ in range(n):
            self.engine.step_begin()
            halo = self._start_halo()                  # travels while the interior segments are computed
            # the scalar is new only when the reduction priced a buffer that changed (every iteration without
            # quirk Q1, every other one with it); the decision is identical on all ranks (same iteration parity)
            if self.world > 1 and self.engine.needs_reduction():
                self._all_reduce_max(self.engine.cfl_slot())
            for req in halo:
                req.wait()                             # domain stream (or the host, with gloo) waits for the rows
            self.engine.step_end()

    def save(self):
        """Device-side checkpoint of this rank's strip (ghost rows included: they are consistent at iteration ends)."""
        self.engine.domain.state_save()

    def restore(self):
        self.engine.domain.state_restore()

    def barrier(self):
        self.engine.sync()
        if self.world > 1:
            self.dist.barrier()
        self.engine.sync()

    def max_over_ranks(self, x):
        if self.world == 1:
            return x
        dev = "cpu" if self.staged else getattr(self.engine, "device", "cpu")
        t = self.torch.tensor([x], dtype=self.torch.float64, device=dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def verify_ghost_rows(self):
        """After a batch: do this strip's ghost rows hold, bit for bit, what their owners hold?  (The exchange follows the
        last iteration of a batch whenever one reach of ghost rows is stored.)  Every rank sends the edge rows it owns to
        the neighbours by torch.distributed -- a channel that has nothing to do with the transport under test -- and
        compares.  Returns the largest number of differing cells any rank found (0 = verified); collective."""
        g, n = self.g, self.local_rows_total
        dom = self.engine.domain
        edges = {}
        if self.south is not None:
            edges[self.south] = dom.download(row0=g, nrows=g)                   # my first owned rows = the south neighbour's north ghost rows
        if self.north is not None:
            edges[self.north] = dom.download(row0=n - 2 * g, nrows=g)
        everyone = [None] * self.world
        self.dist.all_gather_object(everyone, edges)
        bad = 0
        if self.south is not None:
            bad += int((dom.download(row0=0, nrows=g).view(np.uint8) != everyone[self.south][self.rank].view(np.uint8)).reshape(-1, 4 * dom.real().itemsize).any(axis=1).sum())
        if self.north is not None:
            bad += int((dom.download(row0=n - g, nrows=g).view(np.uint8) != everyone[self.north][self.rank].view(np.uint8)).reshape(-1, 4 * dom.real().itemsize).any(axis=1).sum())
        return int(self.max_over_ranks(float(bad)))

    def gather_owned(self):
        """All ranks' owned rows assembled on every rank (tests)."""
        local = self.engine.download()
        mine = np.ascontiguousarray(local[self.own_lo - self.local_lo:self.own_hi - self.local_lo])
        out = [None] * self.world
        self.dist.all_gather_object(out, mine)
        return np.concatenate(out, axis=0)

    # ---- the moving bed: every rank adds every shape with GLOBAL cell ids and keeps the cells on its local rows, ghost rows included
    #      (the library drops the others), so that an apply moves a ghost row exactly as its owner moves the row; nothing is exchanged ----
    def _bed_engine(self, what):
        if not hasattr(self.engine, "bed_apply"):
            raise RuntimeError(f"{what}: this engine has no moving bed (the HIP engine's hp_bed_*)")
        return self.engine

    def bed_shape_add(self, cells, target, series):
        """`cells`: flat ids y * cols + x of the WHOLE grid or (x, y) pairs; every rank calls it with the same arguments."""
        self._bed_engine("bed_shape_add").bed_shape_add(cells, target, series)

    def bed_shapes_clear(self):
        self._bed_engine("bed_shapes_clear").bed_shapes_clear()

    def bed_apply(self):
        """Every rank, between batches.  With two reaches of ghost rows (exchange_period 2) after an even batch only: the library
        refuses an apply while a strip's ghost rows are not all valid."""
        self._bed_engine("bed_apply").bed_apply()

    def gather_bed(self):
        """All ranks' owned rows of the bed assembled on every rank, as gather_owned does for the state (tests)."""
        local = self._bed_engine("gather_bed").download_bed()
        mine = np.ascontiguousarray(local[self.own_lo - self.local_lo:self.own_hi - self.local_lo])
        out = [None] * self.world
        self.dist.all_gather_object(out, mine)
        return np.concatenate(out, axis=0)

    # ---- link groups: every rank adds every group with GLOBAL ids; a strip computes the links whose two ends it stores (ghost rows
    #      included), redundantly with its neighbours, and ignores the others.  A link with exactly one end on a strip cannot run ----
    def add_links(self, links):
        """`links`: see hipims_mi.pack_links; every rank calls it with the same arguments.  Every strip's verdict on every link is
        looked at BEFORE any rank adds anything: a ValueError names the first link some strip would hold one end of."""
        from . import pack_links
        if not hasattr(self.engine, "add_links"):
            raise RuntimeError("add_links: this engine has no link groups (the HIP engine's hp_boundary_add_links)")
        L = pack_links(links, self.cols)
        bad = links_refused(L, self.cols, self.parts, ghost_rows(self.scheme))
        if bad is not None:
            k, rank = bad
            raise ValueError(f"link {k} (cells {int(L['cell_a'][k])} and {int(L['cell_b'][k])}): strip {rank} would hold exactly one of its ends "
                             f"on every iteration (it stores rows {self.parts[rank][2]} to {self.parts[rank][3] - 1})")
        self.engine.add_links(L)                        # (may still refuse the group: only what the engine took is remembered)
        self._links = L if getattr(self, "_links", None) is None else np.concatenate([self._links, L])

    def gather_links(self):
        """The records of all links on rank 0 (an array of hipims_mi.LINK_RECORD_DTYPE, equal to the single domain's
        Domain.links_read() in every bit), None on the other ranks: a link's record is the one of the strip that owns its end a.
        Collective."""
        from . import LINK_RECORD_DTYPE
        L = getattr(self, "_links", None)
        if L is None:
            raise RuntimeError("gather_links: no link group was added")
        rows_a = (L["cell_a"] // np.uint64(self.cols)).astype(np.int64)
        mine = np.flatnonzero((rows_a >= self.own_lo) & (rows_a < self.own_hi))
        parts = self._gather_parts((mine, self.engine.links_read()[mine]))
        if self.rank != 0:
            return None
        out = np.zeros(len(L), LINK_RECORD_DTYPE)
        for idx, rec in parts:
            out[idx] = rec
        return out

    # ---- the open boundary: every rank adds every segment with GLOBAL indices; a strip keeps the ring cells whose row it stores (ghost
    #      rows included) and recomputes the west and east ones on its ghost rows redundantly with their owners ----
    def add_open(self, segments):
        """`segments`: see hipims_mi.pack_open_segments; every rank calls it with the same arguments.  A strip with two reaches of
        ghost rows is refused by the engine (HP_ERR_UNSUPPORTED)."""
        from . import pack_open_segments
        if not hasattr(self.engine, "add_open"):
            raise RuntimeError("add_open: this engine has no open boundary (the HIP engine's hp_boundary_add_open)")
        S = pack_open_segments(segments, self.cols, self.rows)
        self.engine.add_open(S)                         # (may still refuse the segments: only what the engine took is remembered)
        self._open = S if getattr(self, "_open", None) is None else np.concatenate([self._open, S])

    def open_rows(self):
        """The GLOBAL row of every listed ring cell, in the records' order."""
        from . import EDGE_NORTH, EDGE_SOUTH
        rows = []
        for s in self._open:
            n = int(s["last"]) - int(s["first"]) + 1
            if int(s["edge"]) == EDGE_SOUTH:
                rows.append(np.zeros(n, np.int64))
            elif int(s["edge"]) == EDGE_NORTH:
                rows.append(np.full(n, self.rows - 1, np.int64))
            else:
                rows.append(np.arange(int(s["first"]), int(s["last"]) + 1, dtype=np.int64))
        return np.concatenate(rows)

    def gather_open(self):
        """The records of all open cells on rank 0 (an array of hipims_mi.OPEN_RECORD_DTYPE, equal to the single domain's
        Domain.open_read() in every bit), None on the other ranks: a cell's record is the one of the strip that owns its row.
        Collective."""
        from . import OPEN_RECORD_DTYPE
        if getattr(self, "_open", None) is None:
            raise RuntimeError("gather_open: no open segment was added")
        rows = self.open_rows()
        mine = np.flatnonzero((rows >= self.own_lo) & (rows < self.own_hi))
        parts = self._gather_parts((mine, self.engine.open_read()[mine]))
        if self.rank != 0:
            return None
        out = np.zeros(len(rows), OPEN_RECORD_DTYPE)
        for idx, rec in parts:
            out[idx] = rec
        return out

    # ---- the infiltration: every rank adds the rows of the global rasters that it stores, ghost rows included, and recomputes F on its
    #      ghost rows: F is a function of the cell's own history of (Z, dt), which with an exchange after every iteration is its owner's
    #      bit for bit.  Nothing of F is exchanged; with two reaches of ghost rows the outer one is stale every other iteration ----
    def add_infiltration(self, soil_global, classes, initial_global=None):
        """`soil_global`, `initial_global`: the [rows, cols] rasters of the WHOLE grid (row 0 = south); every rank calls it with the
        same arguments.  Refused BEFORE any rank adds anything where the strips exchange after every second iteration only."""
        from . import soil_ids
        if not hasattr(self.engine, "add_infiltration"):
            raise RuntimeError("add_infiltration: this engine has no infiltration (the HIP engine's hp_boundary_add_infiltration)")
        if self.exchange_period > 1 and self.world > 1:
            raise ValueError("add_infiltration: the strips store two reaches of ghost rows and exchange after every second iteration "
                             "(exchange_period = 2): the cumulative infiltration on the outer reach would drift from its owner's; use exchange_period = 1")
        ids = soil_ids(soil_global)
        if ids.shape != (self.rows, self.cols):
            raise ValueError(f"the soil raster must be [{self.rows}, {self.cols}]")
        f0 = None
        if initial_global is not None:
            f0 = np.asarray(initial_global, dtype=np.float64)
            if f0.shape != (self.rows, self.cols):
                raise ValueError(f"the initial infiltration must be [{self.rows}, {self.cols}]")
            f0 = np.ascontiguousarray(f0[self.local_slice()])
        self.engine.add_infiltration(np.ascontiguousarray(ids[self.local_slice()]), classes, f0)
        self._infiltration = True

    # ---- the tracer: a strip has none (hp_tracer_enable answers HP_ERR_UNSUPPORTED: M's ghost rows would need an exchange of their own);
    #      the refusal is the engine's own and is passed through ----
    def tracer_enable(self, initial_global=None):
        """`initial_global`: the [rows, cols] raster of the WHOLE grid (row 0 = south), or None.  On more than one strip the engine
        refuses (hipims_mi.HipimsError, HP_ERR_UNSUPPORTED), and so does this call."""
        if not hasattr(self.engine, "tracer_enable"):
            raise RuntimeError("tracer_enable: this engine has no tracer (the HIP engine's hp_tracer_enable)")
        m0 = None
        if initial_global is not None:
            m0 = np.asarray(initial_global, dtype=np.float64)
            if m0.shape != (self.rows, self.cols):
                raise ValueError(f"the initial tracer must be [{self.rows}, {self.cols}]")
            m0 = np.ascontiguousarray(m0[self.local_slice()])
        self.engine.tracer_enable(m0)

    def gather_infiltration(self):
        """The cumulative infiltration F of the whole grid on rank 0 (fp64 [rows, cols], equal to the single domain's
        Domain.infiltration_read() in every bit), None on the other ranks: every rank's OWNED rows.  Collective."""
        if not getattr(self, "_infiltration", False):
            raise RuntimeError("gather_infiltration: no infiltration was added")
        mine = self.engine.infiltration_read(self.own_lo - self.local_lo, self.own_hi - self.own_lo)
        parts = self._gather_parts(mine)
        return np.concatenate(parts, axis=0) if self.rank == 0 else None

    def gather_outputs(self, values, dtype=np.float64):
        """Output rasters of the whole grid: every rank derives its OWNED rows on its device (Domain.derive), rank 0 gets
        {name: array[rows, cols]}, the other ranks None.  Pickled objects over the process group, as gather_owned; collective."""
        mine = self.engine.derive(values, dtype=dtype, row0=self.own_lo - self.local_lo, nrows=self.own_hi - self.own_lo)
        parts = [None] * self.world if self.rank == 0 else None
        self.dist.gather_object(mine, parts, dst=0)                 # rasters travel to rank 0 only
        return assemble_outputs(parts) if self.rank == 0 else None

    def gather_overview(self, values, aggregates, factor, dtype=np.float64):
        """Block-aggregated overviews of the whole grid (Domain.overview): every rank aggregates its OWNED rows on its device --
        blocks are anchored to the global grid, so a block that a strip border cuts comes in two parts --, rank 0 puts the parts
        together (assemble_overviews) and gets one array [ceil(rows / factor), ceil(cols / factor)] per (value, aggregate) pair,
        equal to the single domain's in every bit; the other ranks None.  Collective."""
        from . import overview_pairs
        pairs = overview_pairs(values, aggregates)
        row0, nrows = self.own_lo - self.local_lo, self.own_hi - self.own_lo
        mine = (self.engine.overview_shape(factor, row0=row0, nrows=nrows)[0],
                self.engine.overview([v for v, _ in pairs], [a for _, a in pairs], factor, dtype=dtype, row0=row0, nrows=nrows))
        parts = self._gather_parts(mine)
        return assemble_overviews(parts, [a for _, a in pairs]) if self.rank == 0 else None

    def gather_sparse(self, values, select="depth", above=0.0, dtype=np.float64):
        """The selected cells of the whole grid in CSR (Domain.sparse): every rank compacts its OWNED rows on its device, rank 0
        concatenates the parts in rank order (frontend.combine_sparse) and gets (row_ptr, col, [one array per value]), equal to
        the single domain's in every word; the other ranks None.  Collective."""
        from . import frontend
        mine = self.engine.sparse(values, select=select, above=above, dtype=dtype, row0=self.own_lo - self.local_lo, nrows=self.own_hi - self.own_lo)
        parts = self._gather_parts(mine)
        return frontend.combine_sparse(parts) if self.rank == 0 else None

    def _gather_parts(self, mine):
        """Every rank's `mine` in rank order on rank 0, None on the other ranks: pickled over the process group, which a single
        rank does not need."""
        if self.world == 1:
            return [mine]
        parts = [None] * self.world if self.rank == 0 else None
        self.dist.gather_object(mine, parts, dst=0)
        return parts

    # ---- the peak tracker: every rank tracks its own strip (ghost rows included: they hold their owners' values between
    #      batches), nothing is exchanged; only owned rows are ever gathered ----
    def peaks_enable(self, values, arrival_depth=0.01):
        self.engine.peaks_enable(values, arrival_depth=arrival_depth)

    def peaks_sample(self):
        self.engine.peaks_sample()

    def gather_peaks(self, values=None, dtype=np.float64):
        """Peak rasters of the whole grid: every rank reads its OWNED rows (Domain.peaks), rank 0 gets {name: array[rows, cols]},
        the other ranks None.  Like gather_outputs; collective."""
        mine = self.engine.peaks(values, dtype=dtype, row0=self.own_lo - self.local_lo, nrows=self.own_hi - self.own_lo)
        parts = [None] * self.world if self.rank == 0 else None
        self.dist.gather_object(mine, parts, dst=0)
        return assemble_outputs(parts) if self.rank == 0 else None

    # ---- the probe recorder: every rank records the points on the rows it owns as gauges (probe_points); rank 0 forms the
    #      sections' discharges from the gathered values (assemble_probes) ----
    def probes_enable(self, gauges=(), sections=(), capacity=4096, dx=None):
        """`gauges`: (x, y) and `sections`: (cells, wx, wy) triples or frontend.rasterise_section's objects, in GLOBAL cell
        indices.  `dx`: the cell size of the discharges (default: the HIP domain's; 1 with another engine)."""
        self._probe_gauges, self._probe_sections, points = probe_points(gauges, sections)
        if (points < 0).any() or (points[:, 0] >= self.cols).any() or (points[:, 1] >= self.rows).any():
            raise ValueError("a probe cell lies outside the grid")
        self._probe_dx = float(dx if dx is not None else (self.domain.desc.dx if self.domain is not None else 1.0))
        self._probe_mine = np.flatnonzero((points[:, 1] >= self.own_lo) & (points[:, 1] < self.own_hi))
        local = points[self._probe_mine] - np.array([0, self.local_lo])
        self._probe_host = None
        if not len(local):
            return                                      # (no point on this rank's rows: nothing to record here)
        if hasattr(self.engine, "probes_enable"):
            self.engine.probes_enable(local, (), capacity=capacity)
        else:                                           # an engine without the device path: the host recorder on the downloaded strip
            from . import frontend
            self._probe_host = frontend.ProbeRecorder(local, ())

    def probes_sample(self):
        if not len(self._probe_mine):
            return
        if self._probe_host is None:
            self.engine.probes_sample()
        else:
            self._probe_host.record(self.engine.download(), self._bed_local, self.engine.scalars()["t"])

    def gather_probes(self):
        """The series of the whole grid: rank 0 gets {"t": [n], "gauges": [n, G, 4], "sections": [n, S]}, bit-identical to the
        single domain's Domain.probes(); the other ranks None.  Pickled objects over the process group; collective."""
        mine = None
        if len(self._probe_mine):
            series = self.engine.probes() if self._probe_host is None else self._probe_host.series()
            mine = (self._probe_mine, series["t"], series["gauges"])
        parts = self._gather_parts(mine)
        return assemble_probes(parts, self._probe_gauges, self._probe_sections, self._probe_dx) if self.rank == 0 else None

    # ---- the zone recorder: every rank records its local rows with the ghost rows' ids set to 0, so that every cell is counted on
    #      exactly one rank; the records are integers, so rank 0's sums and maxima (frontend.combine_zones) are the single domain's ----
    def zones_enable(self, ids_global, zone_count=None, flood_depth=0.1, capacity=4096, dx=None):
        """`ids_global`: the [rows, cols] raster of zone ids of the WHOLE grid (row 0 = south; 0 = in no zone).  `dx`: the cell size
        of the volumes (default: the HIP domain's; 1 with another engine)."""
        from . import frontend
        ids = frontend.zone_ids(ids_global)
        if ids.shape != (self.rows, self.cols):
            raise ValueError(f"the zone raster must be [{self.rows}, {self.cols}]")
        self._zone_count = int(zone_count) if zone_count is not None else max(1, int(ids.max()))
        self._zone_dx = float(dx if dx is not None else (self.domain.desc.dx if self.domain is not None else 1.0))
        local = ids[self.local_slice()].copy()
        local[:self.own_lo - self.local_lo] = 0         # the ghost rows belong to the neighbours
        local[self.own_hi - self.local_lo:] = 0
        self._zone_host, self._zones_on = None, True
        if hasattr(self.engine, "zones_enable"):
            self.engine.zones_enable(local, self._zone_count, flood_depth=flood_depth, capacity=capacity)
        else:                                           # an engine without the device path: the host recorder on the downloaded strip
            self._zone_host = frontend.ZoneRecorder(local, self._zone_count, flood_depth, self._zone_dx)

    def _zones_required(self, what):
        if not getattr(self, "_zones_on", False):
            raise RuntimeError(f"{what}: the zone recorder is not enabled (StripRunner.zones_enable comes first)")

    def zones_sample(self):
        self._zones_required("zones_sample")
        if self._zone_host is None:
            self.engine.zones_sample()
        else:
            self._zone_host.record(self.engine.download(), self._bed_local, self.engine.scalars()["t"])

    def gather_zones(self):
        """The series of the whole grid: rank 0 gets Domain.zones()' dictionary, equal to the single domain's in every word; the
        other ranks None.  Pickled objects over the process group; collective."""
        from . import frontend, split_zone_records
        self._zones_required("gather_zones")
        mine = self.engine.zone_records() if self._zone_host is None else self._zone_host.words()
        parts = self._gather_parts(mine)
        return split_zone_records(frontend.combine_zones(parts), self._zone_count, self._zone_dx) if self.rank == 0 else None

    def gather_stats(self):
        """Domain.stats over the whole grid, on every rank (combine_stats); cell ids are global.  Collective."""
        mine = self.engine.stats(row0=self.own_lo - self.local_lo, nrows=self.own_hi - self.own_lo)
        parts = [None] * self.world
        self.dist.all_gather_object(parts, (mine, self.local_lo))
        return combine_stats([p[0] for p in parts], [p[1] for p in parts], self.cols)

    def close(self, destroy_group=True):
        """`destroy_group=False` keeps the process group for another StripRunner of this process (bench.py's second leg)."""
        if self.loop == "cxx":
            self.domain.strip_comm_destroy()
        self.engine.close()
        if destroy_group and self.dist.is_initialized():
            self.dist.destroy_process_group()
