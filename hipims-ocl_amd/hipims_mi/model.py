"""Orchestrator above the C ABI for ONE Cartesian domain: what `CModel::runModelMain` and
`CSchemeGodunov::runSimulation / Threaded_runBatch` do around the device work -- sync targets clipped to the output
interval, the batch-size autotuner, skipped-iteration handling at sync points, progress / rate reporting and the
output rasters -- restated for a single domain.

    SchemeDriver  ~ CSchemeGodunov's host-side control  (src/Schemes/CSchemeGodunov.cpp:1053-1092, :1147-1453,
                    :1568-1612, :1741-1835)
    Model         ~ CModel::runModelMain for one local domain (src/CModel.cpp:536-698, :723-891, :905-1100)

Note on reproducibility: in the reference the batch size comes from wall-clock timing, and batch boundaries are not
physics-neutral there -- with quirk Q1 the timestep after a sync point is priced on the pre- or post-step buffer
depending on the parity of the iteration that landed on the sync point and on whether skipped iterations followed.
This restatement keeps the mechanism; pass a fixed batch size (`queueMode="fixed"` in the reference) for
repeatable runs (tests/test_frontend.py shows both).

Multi-domain links, forecast/rollback and MPI are deliberately absent: the strip runner (strips.py) replaces them.
The engine is any object with the `Domain` surface; the CPU tests pass an oracle-backed one.
"""
from __future__ import annotations

import math
import os
import time

import numpy as np

from . import OUT_CODES, frontend


def seconds_to_time(s: float) -> str:
    """Util::secondsToTime: d/h/m/s text of the progress block (src/util.cpp:130-172 shape, not byte-for-byte)."""
    s = max(0.0, float(s))
    if s < 60:
        return f"{s:.2f}s" if s < 10 else f"{s:.1f}s"
    d, rem = divmod(int(s), 86400)
    h, rem = divmod(rem, 3600)
    m, sec = divmod(rem, 60)
    out = (f"{d}d " if d else "") + f"{h:02d}:{m:02d}:{sec:02d}"
    return out


def output_file_name(pattern, t, ext, fmt=""):
    """The file of an output at time t: %t is the time in whole seconds, the pattern's extension gives way to `ext` -- under "xml" to
    what the model file asks for: format="HFA" -> Imagine .img, anything else ESRI ASCII."""
    if ext == "xml":
        ext = ".img" if fmt == "HFA" else ".asc"
    return os.path.splitext(pattern.replace("%t", str(int(round(t)))))[0] + ext


class SchemeDriver:
    """Host-side state of one scheme: the part of CSchemeGodunov that decides WHAT to queue."""

    def __init__(self, sim, cfg, cells):
        self.sim, self.cfg = sim, cfg
        self.cells = cells
        # CScheme.cpp:46-55, CSchemeGodunov.cpp:42-75 defaults; single domain: rollback limit "infinite"
        # (CDomainBase.cpp:163-174)
        self.automatic_queue = True
        self.queue_addition_size = 1
        self.rollback_limit = 999999999
        self.running = False
        self.peak_sampler = None                                   # Model's: called after every batch queued (the peak tracker)
        self.samplers = []                                         # ... and these after it, in order (the probe recorder)
        self.bed_stage = None                                      # Model's: called with (t_before, t_after) behind every batch, in front of the samplers (the moving bed)
        self.prepare_simulation()

    # ---- adapters: Domain (HIP engine) and OracleSim spell a few things differently ----
    def _call(self, *names):
        for n in names:
            f = getattr(self.sim, n, None)
            if f is not None:
                return f
        raise AttributeError(names[0])

    def _scalars(self):
        s = self._call("read_scalars", "scalars")()
        if "time" in s:
            return s["time"], s["timestep"], s["batch_timesteps"], s["batch_successful"], s["batch_skipped"]
        return s["t"], s["dt"], s["batch_dt"], s["batch_ok"], s["batch_skipped"]

    def device_time(self):
        """The engine's own time, read now (one read of its scalars)."""
        return self._scalars()[0]

    # CSchemeGodunov::prepareSimulation (:1053-1092)
    def prepare_simulation(self):
        self.target_time = 0.0
        self.current_time = 0.0
        self.current_timestep = self.cfg.timestep
        self.batch_timesteps = 0.0
        self.batch_successful = self.batch_skipped = 0
        self.batch_rate = 1
        self.batch_started = 0.0
        self.iterations_since_sync = 0
        self.cells_calculated = 0
        self.iterations = 0
        self.update_target = False
        self.override_timestep = False
        self.use_forced_time_advance = True
        self.read_key_statistics()

    # :1741-1753
    def set_target_time(self, t):
        if t == self.target_time:
            return
        self.target_time = t
        self.update_target = True

    def force_time_advance(self):
        self.use_forced_time_advance = True

    # :1817-1835
    def read_key_statistics(self):
        last = self.batch_successful
        (self.current_time, self.current_timestep, self.batch_timesteps, self.batch_successful,
         self.batch_skipped) = self._scalars()
        self.batch_rate = (self.batch_successful - last) if self.batch_successful > last else 1

    # :1568-1612 (forecast sync, one domain)
    def is_sync_ready(self, expected_target):
        return not self.running and not (expected_target - self.current_time > 1e-5)

    def is_suspended(self):
        return self.current_timestep < 0.0

    # :1374-1453 followed by one pass of Threaded_runBatch (:1147-1372); blocking here, where the reference hands the
    # pass to its worker thread and polls isRunning()
    def run_simulation(self, target, real_time):
        if self.running:
            return
        if self.target_time != target:
            self.set_target_time(target)
        if target <= 0.0:
            return
        if self.current_time > target + 1e-5:                      # :1389-1407 (a warning in the reference)
            return
        if self.automatic_queue and real_time > 1e-5:              # :1420-1448, single-domain branch
            duration = real_time - self.batch_started
            old = self.queue_addition_size
            if duration > 0:
                want = int(math.ceil(1.0 / (duration / float(old))))
                self.queue_addition_size = max(1, min(self.batch_rate * 3, want))
            if self.queue_addition_size > old * 2 and self.queue_addition_size > 40:
                self.queue_addition_size = min(self.batch_rate * 3, old * 2)
            self.queue_addition_size = min(self.queue_addition_size, self.rollback_limit - self.iterations_since_sync)
            self.queue_addition_size = max(1, self.queue_addition_size)
        self.batch_started = real_time
        self.running = True
        stats_read = False
        try:
            if self.update_target:                                 # :1163-1209
                self.update_target = False
                self._call("set_target_time", "set_target")(self.target_time)
                self.iterations_since_sync = 0
                self.use_forced_time_advance = True
                if self.current_timestep <= 0.0:                   # a suspended scheme needs a new timestep: queued on the
                    self._call("update_timestep")()                # device; the host copy is NOT refreshed before the
                                                                   # test below (as in the reference, :1189-1200)
                if self.current_time + self.current_timestep > self.target_time + 1e-5:
                    self.current_timestep = self.target_time - self.current_time
                    self.override_timestep = True
            if self.current_time < self.target_time and self.override_timestep:    # :1213-1232
                self._call("force_timestep", "force_dt")(self.current_timestep)
                self.override_timestep = False
            if self.iterations_since_sync < self.rollback_limit and self.current_time < self.target_time:   # :1285-1304
                n = self.queue_addition_size
                t_before = self.current_time
                self._call("step_batch", "run")(n)
                self.iterations_since_sync += n
                self.iterations += n
                self.cells_calculated += n * self.cells            # :1299: cols x rows per iteration, skipped or not
                if self.bed_stage is not None:                     # the bed moves before anything samples: the statistics are read here
                    self.read_key_statistics()                     # instead of below (an apply changes none of them)
                    stats_read = True
                    self.bed_stage(t_before, self.current_time)
                if self.peak_sampler is not None:                  # one sample per batch, queued behind it (no reference counterpart)
                    self.peak_sampler()
                for sampler in self.samplers:
                    sampler()
            if not stats_read:
                self.read_key_statistics()                         # :1309-1313, blockUntilFinished, :1350
        finally:
            self.running = False


class Model:
    """CModel for one domain: `run()` is runModelMain.

    The zone recorder's arguments: `zones` is the raster of zone ids ([rows, cols] array, row 0 = south, or a raster file;
    default: the model file's "zones" data source), `zone_flood_depth` the "flooded" threshold in metres, `zone_capacity` the
    number of samples the device buffer holds before it is drained to the host (as `probe_capacity` for the probes; clamped to
    what fits the recorder's 256 MiB limit; it changes when the buffer is drained, never what is recorded)."""

    def __init__(self, xml_path, make_sim=None, output_format=".npy", log=None, progress_interval=0.85,
                 clock=time.perf_counter, device_outputs=None, peaks=None, peak_arrival_depth=0.01, gauges=None, sections=None,
                 probe_capacity=4096, zones=None, zone_flood_depth=0.1, zone_capacity=4096, overviews=None, sparse=None, bed_shapes=None,
                 links=None, infiltration=None, tracer=None, open_edges=None, tracers=None):
        """The engine and one _setup_* call per feature.  Their order is the order of the engine's calls: the file's boundaries, then
        what else acts inside an iteration in the order it acts there, the tracer last (behind everything that may refuse it); then
        the observers in the order they sample, and the moving bed, whose first apply comes in front of every observer's first sample."""
        self.cfg = cfg = frontend.parse_configuration(xml_path)
        self.state0, self.bed, self.manning, self.res = frontend.build_domain(cfg)
        self.rows, self.cols = self.bed.shape
        self.output_format, self.log, self.clock = output_format, log, clock
        self.sim = self._make_engine(make_sim)
        self.sim.upload(self.state0, self.bed, self.manning)
        frontend.attach_boundaries(cfg, self.sim, self.cols)
        self._setup_links(links)
        self._setup_open(open_edges)
        self._setup_infiltration(infiltration)
        self._setup_tracers(tracer, tracers)
        self.scheme = SchemeDriver(self.sim, cfg, self.cols * self.rows)
        self.progress_interval = progress_interval
        self.simulation_time = cfg.duration                        # dSimulationTime
        self.output_frequency = cfg.output_frequency
        self.current_time = self.target_time = self.last_sync_time = self.last_output_time = 0.0
        self.last_progress = 0.0
        self.outputs = []                                          # [(time, {value: array})]
        self.progress_blocks = []
        self._setup_outputs_path(device_outputs)
        self._setup_peaks(peaks, peak_arrival_depth)
        self._setup_probes(gauges, sections, probe_capacity)
        self._setup_zones(zones, zone_flood_depth, zone_capacity)
        self._setup_overviews(overviews)
        self._setup_sparse(sparse)
        self._setup_beds(bed_shapes)
        self.domain_stats = []                                     # [(time, stats())]: start, then every output time
        self.log_domain_stats(initial=True)

    # ---- what the setup methods share ----
    def _make_engine(self, make_sim):
        cfg = self.cfg
        if make_sim is not None:
            return make_sim(cfg, self.cols, self.rows, self.res)
        from . import Domain
        return Domain(self.cols, self.rows, dx=self.res, scheme=cfg.scheme, precision=cfg.precision,
                      dry_threshold=cfg.dry_threshold, courant=cfg.courant, t_end=cfg.duration,
                      dynamic_dt=cfg.dynamic_dt, dt_fixed=cfg.timestep, dt_initial=cfg.timestep,
                      friction=cfg.friction, device=cfg.device_number - 1)

    def _raster(self, given, noun, dtype=None):
        """A raster argument -- a file or an array -- as an array of the domain's shape; `noun` names it where it is refused."""
        a = frontend.read_raster(given)[0] if isinstance(given, (str, os.PathLike)) else np.asarray(given, dtype=dtype)
        if a.shape != (self.rows, self.cols):
            raise ValueError(f"{noun} is {a.shape[1]} x {a.shape[0]} cells, the domain {self.cols} x {self.rows}")
        return a

    def _require(self, method, sentence):
        """What acts inside every iteration needs an engine that has it on the device."""
        if not hasattr(self.sim, method):
            raise NotImplementedError(sentence)

    def _data_source(self, value, noun):
        """The file of the model file's <dataSource type="raster" value=...> of that value, or None."""
        source = next((src for src in self.cfg.sources if value in src[1]), None)
        if source is None:
            return None
        if source[0] != "raster":
            raise ValueError(f"the {noun} data source must be a raster")
        return os.path.join(self.cfg.source_dir, source[2])

    def _warn_inert(self, what):
        if self.cfg.scheme == frontend.SCHEME_MUSCL_HANCOCK and self.log:
            self.log(f"Warning: {what} inert under MUSCL-Hancock, like every boundary condition (quirk Q8)")

    @staticmethod
    def _tracer_sources(sources):
        return [dict(cells=list(s["cells"]), series=np.asarray(s["series"], dtype=np.float64).reshape(-1, 2)) for s in (sources or [])]

    # ---- what acts inside every iteration ----
    def _setup_links(self, links):
        """Link groups (no reference counterpart): the rows of the model file's <links mapFile="links.csv"/> elements inside
        <boundaryConditions> and the dict(a=(x, y), b=(x, y), kind=, one_way=, level=, size=, coeff=, limit=) entries of `links`, one
        group behind the file's boundaries.  They act inside every iteration, so only an engine that has them on the device will do."""
        self.link_list = [dict(l) for l in list(self.cfg.links) + list(links or [])]
        self.link_series = []                                      # [(time, records)]: one entry per output time
        if self.link_list:
            self._require("add_links", "link groups act inside every iteration: they need an engine with add_links (the HIP engine)")
            self._warn_inert("link groups are")
            self.sim.add_links(self.link_list)

    def _setup_open(self, open_edges):
        """The open boundary (no reference counterpart): the model file's <domainEdge edge="east" treatment="open" name="outlet" from="8"
        to="23"/> elements and the dict(edge=, name=, first=, last=) entries (or bare edge names) of `open_edges`, one call behind the
        file's boundaries and the links.  It acts inside every iteration, so only an engine that has it on the device will do."""
        self.open_list = []
        for k, e in enumerate(list(self.cfg.open_edges) + list(open_edges or [])):
            e = dict(edge=e) if isinstance(e, str) else dict(e)
            e.setdefault("name", f"{e['edge']}{k}")
            self.open_list.append(e)
        self.open_series = []                                      # [(time, [(discharge, volume) per segment])]: one entry per output time
        if self.open_list:
            from . import pack_open_segments
            self._require("add_open", "the open boundary acts inside every iteration: it needs an engine with add_open (the HIP engine)")
            segments = pack_open_segments([dict(edge=e["edge"], first=e.get("first"), last=e.get("last")) for e in self.open_list], self.cols, self.rows)
            self.open_segment_of = np.concatenate([np.full(int(s["last"]) - int(s["first"]) + 1, k) for k, s in enumerate(segments)])
            self.sim.add_open(segments)

    def _setup_infiltration(self, infiltration):
        """The infiltration (no reference counterpart): the raster of a <dataSource type="raster" value="soil" source="..."/> with the
        classes of <soilClasses source="soil.csv"/> (columns ks, suction, deficit, capacity), or `infiltration`: dict(soil=, classes=,
        initial=) with soil an array [rows, cols] (row 0 = south; 0 = impervious) or a raster file.  Behind the file's boundaries and
        the links, so the rain of an iteration is on the ground before the soil takes its share.  It acts inside every iteration, so
        only an engine that has it on the device will do.  A <dataTarget value="infiltration" .../> writes F at every output time."""
        spec = dict(infiltration) if infiltration else None
        if spec is None:
            source = self._data_source("soil", "soil")
            if source is not None:
                if not self.cfg.soil_classes:
                    raise ValueError("the soil data source needs a <soilClasses source=.../> element")
                spec = dict(soil=source, classes=self.cfg.soil_classes)
        self.infiltration = None
        if spec is not None:
            soil = self._raster(spec["soil"], "the soil raster")
            self._require("add_infiltration", "the infiltration acts inside every iteration: it needs an engine with add_infiltration (the HIP engine)")
            self._warn_inert("the infiltration is")
            self.infiltration = dict(soil=soil, classes=list(spec["classes"]), initial=spec.get("initial"))
            self.sim.add_infiltration(soil, self.infiltration["classes"], self.infiltration["initial"])
        elif any(what == "infiltration" for what, _ in self.cfg.targets):
            raise ValueError("an infiltration data target needs a soil data source")

    def _setup_tracers(self, tracer, tracers):
        """The tracer (no reference counterpart): the initial M of a <dataSource type="raster" value="tracer" source="m0.asc"/> and the
        sources of the <tracerSource mapFile="cells.csv" source="rate.csv"/> elements, or `tracer`: dict(initial=, sources=[dict(cells=,
        series=)]) with initial an array [rows, cols] (row 0 = south), a raster file or None.  Enabled behind everything that may refuse
        it.  It moves inside every iteration, so only an engine that has it on the device will do.  A <dataTarget value="tracer" .../>
        writes M at every output time, a <dataTarget value="concentration" .../> M / h (frontend.tracer_concentration).
        A tracer SET: the <tracerSpecies name= decay= source=/> elements with their <tracerSource species=.../>, or `tracers`: [dict(name=,
        initial=, decay=, sources=[dict(cells=, series=)])]: one run of the water carries them all (hp_tracer_enable_set).  Targets name
        their species (<dataTarget value="tracer|concentration" species=.../>) and their files carry its name.  Either form, not both."""
        cfg = self.cfg
        species = [dict(t) for t in tracers] if tracers is not None else None
        if species is None and cfg.tracer_species:
            species = [dict(name=t["name"], decay=t["decay"], initial=os.path.join(cfg.source_dir, t["initial"]) if t["initial"] else None,
                            sources=[s for s in cfg.tracer_sources if s.get("species") == t["name"]], exchange=t.get("exchange"),
                            deposit=os.path.join(cfg.source_dir, t["deposit"]) if t.get("deposit") else None) for t in cfg.tracer_species]
        spec = dict(tracer) if tracer is not None else None
        source = next((src for src in cfg.sources if "tracer" in src[1]), None)
        unnamed = [s for s in cfg.tracer_sources if s.get("species") is None]
        if species is not None and (spec is not None or (tracers is None and (source is not None or unnamed))):
            raise ValueError("a single tracer (tracer=, a tracer data source, a <tracerSource> without species) and a tracer set "
                             "(tracers=, <tracerSpecies>) are given: a domain carries one or the other")
        if species is None and any(s.get("species") is not None for s in cfg.tracer_sources):
            raise ValueError("a <tracerSource species=...> needs its <tracerSpecies> element")
        self.tracer_set = self.tracer = None
        if species is not None:
            self._enable_tracer_set(species, from_file=tracers is None)
        self._check_tracer_targets()
        if self.tracer_set is not None:
            return
        if spec is None and (source is not None or cfg.tracer_sources):
            spec = dict(initial=self._data_source("tracer", "tracer"), sources=cfg.tracer_sources)
        if spec is not None:
            m0 = spec.get("initial")
            if m0 is not None:
                m0 = self._raster(m0, "the tracer raster", np.float64)
            self._require("tracer_enable", "the tracer moves inside every iteration: it needs an engine with tracer_enable (the HIP engine)")
            self.tracer = dict(initial=m0, sources=self._tracer_sources(spec.get("sources")))
            self.sim.tracer_enable(m0)
            for s in self.tracer["sources"]:
                self.sim.tracer_add_source(s["cells"], s["series"])
        elif any(what in ("tracer", "concentration") for what, _ in cfg.targets):
            raise ValueError("a tracer or concentration data target needs a tracer (a tracer data source, a <tracerSource> element or Model(tracer=...))")

    def _enable_tracer_set(self, species, from_file):
        """The set of _setup_tracers: its planes and decay rates in one call, every species' sources, then the exchanges."""
        names = [t.get("name") or f"species{k}" for k, t in enumerate(species)]
        if len(set(names)) != len(names):
            raise ValueError("two tracer species of one name")
        for s in self.cfg.tracer_sources:
            if from_file and s.get("species") not in names:
                raise ValueError(f"a <tracerSource> names the species {s.get('species')!r}, which no <tracerSpecies> declares")
        planes = np.zeros((len(species), self.rows, self.cols))
        for k, t in enumerate(species):
            if t.get("initial") is not None:
                planes[k] = self._raster(t["initial"], f"the raster of species {names[k]!r}", np.float64)
        self._require("tracer_enable_set", "a tracer set moves inside every iteration: it needs an engine with tracer_enable_set (the HIP engine)")
        self.tracer_set = dict(names=names, decay=[float(t.get("decay") or 0.0) for t in species], initial=planes,
                               sources=[self._tracer_sources(t.get("sources")) for t in species])
        self.sim.tracer_enable_set(initial=planes, decay=self.tracer_set["decay"])
        for k, sources in enumerate(self.tracer_set["sources"]):
            for s in sources:
                self.sim.tracer_add_source(s["cells"], s["series"], species=k)
        self._set_tracer_exchanges(species)

    def _set_tracer_exchanges(self, species):
        """A species may settle onto the ground and be picked up again (hp_tracer_set_exchange): <tracerSpecies ... settling= tauDeposit=
        tauErode= erodibility= deposit="d0.asc"/>, or exchange=dict(settling=, tau_deposit=, tau_erode=, erodibility=) and deposit= (an array,
        a raster file or None) in its dict; <dataTarget value="deposit" species=.../> writes its deposit D at every output time.  An
        exchange dict (an empty one: the defaults) or a deposit asks for it."""
        self.tracer_set["exchange"] = [None] * len(species)
        for k, t in enumerate(species):
            if t.get("exchange") is None and t.get("deposit") is None:
                continue
            d0 = t.get("deposit")
            if d0 is not None:
                d0 = self._raster(d0, f"the deposit raster of species {self.tracer_set['names'][k]!r}", np.float64)
            q = {name: float(v) for name, v in frontend.Tracer.exchange_params(dict(t.get("exchange") or {})).items()}
            self._require("tracer_set_exchange", "a species that settles exchanges inside every iteration: it needs an engine with tracer_set_exchange (the HIP engine)")
            self.tracer_set["exchange"][k] = dict(deposit=d0, **q)
            self.sim.tracer_set_exchange(k, deposit=d0, **q)

    def _species_index(self, k):
        """The index in the tracer set of the species that <dataTarget> k names (None: no such species, or no set)."""
        name = self.cfg.target_species[k]
        return self.tracer_set["names"].index(name) if self.tracer_set is not None and name in self.tracer_set["names"] else None

    def _check_tracer_targets(self):
        for k, (what, _) in enumerate(self.cfg.targets):
            name, index = self.cfg.target_species[k], self._species_index(k)
            if what in ("tracer", "concentration") and self.tracer_set is not None and index is None:
                raise ValueError(f"a {what} data target of a tracer set must name one of its species ({name!r})")
            if what in ("tracer", "concentration") and self.tracer_set is None and name is not None:
                raise ValueError(f"a {what} data target names the species {name!r}, and the model has no tracer set")
            if what == "deposit" and (index is None or self.tracer_set["exchange"][index] is None):
                raise ValueError(f"a deposit data target must name a species of the tracer set that exchanges with the bed ({name!r})")

    # ---- the observers ----
    def _setup_outputs_path(self, device_outputs):
        """Where the output rasters are derived: on the device by the engine's `derive` (no state download) or on the host from
        the downloaded state.  None = the device wherever the engine has `derive` AND the domain is fp64 (11-18x faster,
        profiles/r07_output_stage.txt).  An fp32 domain keeps the host path by default: the front end's bed is fp64 (4-decimal
        values, mostly not fp32 numbers) and derive_output takes Z - bed with THAT bed, the device with the fp32 bed it was
        given, so the rasters of a single-precision model file would change.  True / False force a path (True on an fp32
        domain: rasters of the bed the domain holds).  Engines without `derive` (the oracle of the CPU tests): the host path."""
        if device_outputs and not hasattr(self.sim, "derive"):
            raise ValueError("device_outputs=True needs an engine with derive()")
        self.device_outputs = (hasattr(self.sim, "derive") and self.cfg.precision == "f64") if device_outputs is None else bool(device_outputs)

    def _setup_peaks(self, peaks, arrival_depth):
        """The peak tracker (no reference counterpart): on for the <dataTarget> values that are peak names (frontend.peak_value_code)
        and for the names in `peaks`; one sample after every batch.  On the device (Domain.peaks_*) wherever the output rasters
        are derived there, for the same reason; otherwise frontend.PeakTracker on the downloaded state with the front end's bed."""
        self.peak_names = []
        for what in peaks or []:
            if frontend.peak_value_code(what) is None:
                raise ValueError(f"unknown peak value {what}")
        for what in [w for w, _ in self.cfg.targets] + list(peaks or []):
            code = frontend.peak_value_code(what)
            if code is not None and code not in self.peak_names:
                self.peak_names.append(code)
        self.host_peaks, self.device_peaks = None, False
        if self.peak_names:
            self.device_peaks = self.device_outputs and hasattr(self.sim, "peaks_enable")
            if self.device_peaks:
                self.sim.peaks_enable(self.peak_names, arrival_depth=arrival_depth)
                self.scheme.peak_sampler = self.sim.peaks_sample
            else:
                self.host_peaks = frontend.PeakTracker(self.rows, self.cols, arrival_depth, t=self.scheme.current_time)
                self.scheme.peak_sampler = self.sample_peaks_on_host

    def _setup_probes(self, gauges, sections, capacity):
        """The probe recorder (no reference counterpart): the model file's <gauge> and <section> elements and those of `gauges`
        ({name: (x, y)} or (name, x, y) tuples) and `sections` ({name: ((x0, y0), (x1, y1))} or (name, (x0, y0), (x1, y1))), in
        cell indices; one sample after every batch, gauges.csv and sections.csv rewritten at every output time and at the end.
        On the device (Domain.probes_*) wherever the output rasters are derived there; otherwise frontend.ProbeRecorder on the
        downloaded state with the front end's bed."""
        named = lambda extra: [(k,) + tuple(v) for k, v in extra.items()] if isinstance(extra, dict) else [tuple(e) for e in extra or []]
        self.gauge_list = [(n, int(x), int(y)) for n, x, y in list(self.cfg.gauges) + named(gauges)]
        self.section_list = []
        for e in list(self.cfg.sections) + named(sections):
            p0, p1 = ((e[1], e[2]), (e[3], e[4])) if len(e) == 5 else (e[1], e[2])
            self.section_list.append((e[0], frontend.rasterise_section(p0, p1)))
        for what, pts in [("gauge", [(n, x, y) for n, x, y in self.gauge_list])] + \
                [("section", [(n, int(x), int(y)) for x, y in sec.cells]) for n, sec in self.section_list]:
            for n, x, y in pts:
                if not (0 <= x < self.cols and 0 <= y < self.rows):
                    raise ValueError(f"{what} {n}: cell ({x}, {y}) lies outside the domain")
        self.host_probes, self.device_probes = None, False
        if self.gauge_list or self.section_list:
            xy, secs = [(x, y) for _, x, y in self.gauge_list], [sec for _, sec in self.section_list]
            self.device_probes = self.device_outputs and hasattr(self.sim, "probes_enable")
            if self.device_probes:
                self.sim.probes_enable(xy, secs, capacity=capacity)
                self.scheme.samplers.append(self.sim.probes_sample)
            else:
                self.host_probes = frontend.ProbeRecorder(xy, secs, self.res)
                self.scheme.samplers.append(self.sample_probes_on_host)

    def _setup_zones(self, zones, flood_depth, capacity):
        """The zone recorder (no reference counterpart): the raster of a <dataSource type="raster" value="zones" source="..."/> of
        the model file, or `zones` (an array [rows, cols], row 0 = south, or a raster file); integers 0..4096, 0 = in no zone.  One
        sample after every batch, zones.csv rewritten at every output time and at the end.  On the device (Domain.zones_*) wherever
        the output rasters are derived there -- fp32 model files included when device_outputs is forced: the recorder widens the
        values itself --; otherwise frontend.ZoneRecorder on the downloaded state with the front end's bed."""
        if zones is None:
            zones = self._data_source("zones", "zones")
        self.zone_ids, self.host_zones, self.device_zones = None, None, False
        if zones is not None:
            self.zone_ids = frontend.zone_ids(self._raster(zones, "the zone raster"))
            self.zone_count = max(1, int(self.zone_ids.max()))
            self.device_zones = self.device_outputs and hasattr(self.sim, "zones_enable")
            if self.device_zones:                                  # (a record buffer of at most 256 MiB: it is drained when full)
                fits = (256 << 20) // (8 * (1 + 7 * self.zone_count))
                self.sim.zones_enable(self.zone_ids, self.zone_count, flood_depth=flood_depth, capacity=max(1, min(int(capacity), fits)))
                self.scheme.samplers.append(self.sim.zones_sample)
            else:
                self.host_zones = frontend.ZoneRecorder(self.zone_ids, self.zone_count, flood_depth, self.res)
                self.scheme.samplers.append(self.sample_zones_on_host)

    def _setup_overviews(self, overviews):
        """Overviews (no reference counterpart): the <dataTarget overview="16" aggregate="max|min|count"> elements of the model file
        and the (value, aggregate, factor) triples of `overviews`; at every output time each is the value's raster aggregated over
        blocks of factor x factor cells, written through write_raster with resolution factor * dx.  On the device
        (Domain.overview) wherever the output rasters are derived there; otherwise frontend.overview of the host derivation."""
        self.overview_list = [tuple(o) for o in self.cfg.overviews] + \
            [(str(v).lower(), frontend.aggregate_name(a), int(f), None, "") for v, a, f in overviews or []]
        for what, _, factor, _, _ in self.overview_list:
            if frontend.data_value_code(what) not in OUT_CODES:
                raise ValueError(f"unknown output {what}")
            if not 1 <= factor <= 4096:
                raise ValueError(f"overview of {what}: factor outside 1..4096")
        self.device_overviews = bool(self.overview_list) and self.device_outputs and hasattr(self.sim, "overview")

    def _setup_sparse(self, sparse):
        """The selected cells (no reference counterpart): the model file's <sparseTarget select="depth" above="0.01"
        values="depth,velocityx,velocityy" target="sparse_%t.npz"/> or `sparse` (a dict of select, above, values and optionally
        target); one selection per model.  At every output time the values at the cells whose `select` value lies above `above`,
        in CSR, written as one .npz (row_ptr, col, one array per value, shape, nodata, select, above).  On the device
        (Domain.sparse) wherever the output rasters are derived there; otherwise frontend.sparse of the host derivation."""
        self.sparse_spec = None
        if sparse is not None or self.cfg.sparse is not None:
            spec = dict(self.cfg.sparse or {}, **(sparse or {}))
            values = spec.get("values") or [spec.get("select", "depth")]
            values = [values] if isinstance(values, str) else list(values)
            self.sparse_spec = spec = dict(select=str(spec.get("select", "depth")).lower(), above=float(spec.get("above", 0.0)),
                                           values=[str(v).lower() for v in values], target=spec.get("target"))
            codes = [frontend.data_value_code(v) for v in spec["values"]]
            for what in [spec["select"]] + spec["values"]:
                if frontend.data_value_code(what) not in OUT_CODES:
                    raise ValueError(f"unknown output {what}")
            if len(set(codes)) != len(codes):
                raise ValueError("sparse: a value is listed twice")
            if math.isnan(spec["above"]):
                raise ValueError("sparse: above is a NaN")
        self.device_sparse = self.sparse_spec is not None and self.device_outputs and hasattr(self.sim, "sparse")

    def _setup_beds(self, bed_shapes):
        """The moving bed (no reference counterpart): the model file's <bedShape name="breach" mapFile="cells.csv" source="progress.csv"/>
        elements (mapFile rows: x, y, target elevation; source rows: time, fraction) and the dict(cells=, target=, series=) entries
        of `bed_shapes`.  One apply after the initial upload, then one behind every batch in which a shape can have moved, always
        in front of the observers' samples: a sample sees the bed of its time.  On the device (Domain.bed_apply) wherever the
        engine has it; otherwise frontend.BedShapes on the downloaded state, uploaded again."""
        self.bed_shape_list = [dict(b) for b in list(self.cfg.bed_shapes) + list(bed_shapes or [])]
        self.host_beds, self.device_beds, self.bed_applies = None, False, 0
        if self.bed_shape_list:
            self.device_beds = hasattr(self.sim, "bed_apply")
            if not self.device_beds:
                self.host_beds = frontend.BedShapes(self.rows, self.cols)
                self._bed_real = np.ascontiguousarray(self.bed, dtype=self.sim.download().dtype)      # the bed as the engine holds it
            for b in self.bed_shape_list:
                b["series"] = np.array(b["series"], dtype=np.float64).reshape(-1, 2)
                if self.device_beds:
                    self.sim.bed_shape_add(b["cells"], b["target"], b["series"])
                else:
                    self.host_beds.add(b["cells"], b["target"], b["series"], bed=self._bed_real)
            self.apply_bed()
            self.scheme.bed_stage = self.bed_stage

    def bed_stage(self, t_before, t_after):
        """Behind a batch from t_before to t_after: an apply iff some shape can have moved in it."""
        if any(t_after > b["series"][0, 0] and t_before < b["series"][-1, 0] for b in self.bed_shape_list):
            self.apply_bed()

    def apply_bed(self):
        if self.device_beds:
            self.sim.bed_apply()
            if not self.device_outputs:                            # whatever is derived on the host takes the bed the domain holds now
                self.bed = self.sim.download(1).astype(np.float64)
        else:
            t = self.scheme.device_time()
            state = np.ascontiguousarray(self.sim.download())
            self.host_beds.apply(state, self._bed_real, t)
            self.sim.upload(state, self._bed_real)                 # (always: an apply IS the two uploads, whatever it moved)
            self.bed = self._bed_real.astype(np.float64)
        self.bed_applies += 1

    def _sample_on_host(self, take):
        """One host sample: the engine's time is read in front of its state."""
        t = self.scheme.device_time()
        take(self.sim.download(), self.bed, t)

    def sample_peaks_on_host(self):
        self._sample_on_host(self.host_peaks.fold)

    def sample_probes_on_host(self):
        self._sample_on_host(self.host_probes.record)

    def sample_zones_on_host(self):
        self._sample_on_host(self.host_zones.record)

    def probes(self):
        """{"t": [n], "gauges": [n, G, 4], "sections": [n, S]}: one entry per batch so far (None without gauges and sections)."""
        if self.host_probes is not None:
            return self.host_probes.series()
        return self.sim.probes() if self.device_probes else None

    def write_probes(self):
        if (self.host_probes is not None or self.device_probes) and self.cfg.target_dir and self.output_format:
            frontend.write_probe_files(self.cfg.target_dir, self.probes(), [n for n, _, _ in self.gauge_list],
                                       [n for n, _ in self.section_list])

    def zones(self):
        """The zone series so far (split_zone_records' dictionary): one entry per batch (None without a zone raster)."""
        if self.host_zones is not None:
            return self.host_zones.series()
        return self.sim.zones() if self.device_zones else None

    def write_zones(self):
        if (self.host_zones is not None or self.device_zones) and self.cfg.target_dir and self.output_format:
            frontend.write_zone_file(self.cfg.target_dir, self.zones(), self.res)

    def _write_series_csv(self, name, columns, series):
        """`name` in the target directory: the header t and `columns`, then a row per output time of `series` [(t, [values])], every
        number in its shortest exact decimal form (repr)."""
        if self.cfg.target_dir and self.output_format:
            os.makedirs(self.cfg.target_dir, exist_ok=True)
            with open(os.path.join(self.cfg.target_dir, name), "w") as f:
                f.write(",".join(["t"] + columns) + "\n")
                for t, values in series:
                    f.write(",".join(repr(float(v)) for v in [t] + list(values)) + "\n")

    def write_links(self):
        """links.csv in the target directory: a row per output time, t, then q_last and volume of every link in the order given."""
        if not self.link_list:
            return
        self.link_series.append((self.current_time, self.sim.links_read()))
        self._write_series_csv("links.csv", [f"{column}_{k}" for k in range(len(self.link_list)) for column in ("q_last", "volume")],
                               [(t, [r[column] for r in rec for column in ("q_last", "volume")]) for t, rec in self.link_series])

    def write_outflow(self):
        """outflow.csv in the target directory: a row per output time, t, then discharge and cumulative volume of every open segment in
        the order given -- math.fsum over the segment's cell records: exactly rounded, so independent of any order."""
        if not self.open_list:
            return
        rec = self.sim.open_read()
        self.open_series.append((self.current_time, [(math.fsum(rec["q_last"][self.open_segment_of == k]), math.fsum(rec["volume"][self.open_segment_of == k]))
                                                     for k in range(len(self.open_list))]))
        self._write_series_csv("outflow.csv", [f"{column}_{e['name']}" for e in self.open_list for column in ("discharge", "volume")],
                               [(t, [v for pair in totals for v in pair]) for t, totals in self.open_series])

    def peaks(self):
        """{name: array} of the tracked peak values so far."""
        if not self.peak_names:
            return {}
        if self.host_peaks is not None:
            all_of_them = self.host_peaks.rasters()
            return {name: all_of_them[name] for name in self.peak_names}
        return self.sim.peaks(self.peak_names)

    # CModel::runModelUpdateTarget (:723-770), one domain: run free until the next output is due
    def update_target(self):
        proposal = self.simulation_time
        if math.floor(proposal / self.output_frequency) > math.floor(self.last_sync_time / self.output_frequency):
            proposal = (math.floor(self.last_sync_time / self.output_frequency) + 1) * self.output_frequency
        self.target_time = proposal

    # ---- the outputs of one output time: gathered, then written ----
    def _output_state(self):
        """The downloaded state of this output time: fetched when it is first asked for, and once."""
        if self._state_now is None:
            self._state_now = self.sim.download()
        return self._state_now

    def _gather_plain(self, plain):
        """{value: raster} of the targets derived from the state: on the device every one in ONE call, rasters only over the host link."""
        if self.device_outputs:
            return self.sim.derive(plain) if plain else {}
        if not self.cfg.targets:                                   # (a model file without a target fetches the state all the same)
            self._output_state()
        return {what: frontend.derive_output(what, self._output_state(), self.bed, self.res) for what in plain}

    def _gather_overviews(self):
        """{(value, aggregate, factor): array}: on the device one call per factor, coarse rasters only over the host link."""
        overviews = {}
        if self.device_overviews:
            for factor in sorted({o[2] for o in self.overview_list}):
                mine = [o for o in self.overview_list if o[2] == factor]
                arrays = self.sim.overview([o[0] for o in mine], [o[1] for o in mine], factor)
                overviews.update({o[:3]: a for o, a in zip(mine, arrays)})
        else:
            for what, aggregate, factor, _, _ in self.overview_list:
                overviews[(what, aggregate, factor)] = frontend.overview(frontend.derive_output(what, self._output_state(), self.bed, self.res), factor, aggregate)
        return overviews

    def _gather_selection(self):
        """(row_ptr, col, [values]) of the selected cells, or None: on the device the selected entries only over the host link."""
        spec = self.sparse_spec
        if self.device_sparse:
            return self.sim.sparse(spec["values"], spec["select"], spec["above"])
        if spec is None:
            return None
        derive = lambda what: frontend.derive_output(what, self._output_state(), self.bed, self.res)
        return frontend.sparse([derive(v) for v in spec["values"]], derive(spec["select"]), spec["above"])

    def _target_array(self, k, what, derived, peaks):
        """-> (the raster of <dataTarget> k, the name of its species or None): a peak so far, the engine's own raster -- the cumulative
        infiltration F; M, M / h or D of the tracer or of the target's species --, or one of the derived ones."""
        if frontend.peak_value_code(what) is not None:
            return peaks[frontend.peak_value_code(what)], None
        if what == "infiltration":
            return self.sim.infiltration_read(), None
        if what not in ("tracer", "concentration", "deposit"):
            return derived[what], None
        index = self._species_index(k)
        if what == "deposit":
            arr = self.sim.tracer_deposit_read(species=index)
        else:
            arr = self.sim.tracer_read() if index is None else self.sim.tracer_read(species=index)
        if what == "concentration":
            arr = frontend.tracer_concentration(arr, self.sim.download(), self.sim.download_bed() if hasattr(self.sim, "download_bed") else self.bed)
        return arr, (None if index is None else self.tracer_set["names"][index])

    @staticmethod
    def _species_pattern(pattern, species):
        """The file of a species' raster carries the species' name: at %s, else in front of %t, else last."""
        stem, tail = os.path.splitext(pattern)
        if "%s" in pattern:
            return pattern.replace("%s", species)
        if species in stem:
            return pattern
        return (stem.replace("%t", species + "_%t", 1) if "%t" in stem else stem + "_" + species) + tail

    def _write_raster(self, pattern, arr, resolution, fmt):
        if pattern and self.cfg.target_dir and self.output_format:
            fname = output_file_name(pattern, self.current_time, self.output_format, fmt)
            frontend.write_raster(os.path.join(self.cfg.target_dir, fname), arr, resolution)

    def _write_selection(self, selection):
        """-> the "sparse" entry of the outputs; its .npz where the selection has a target."""
        spec = self.sparse_spec
        entry = dict(row_ptr=selection[0], col=selection[1], **dict(zip(spec["values"], selection[2])))
        if spec["target"] and self.cfg.target_dir and self.output_format:
            os.makedirs(self.cfg.target_dir, exist_ok=True)
            np.savez(os.path.join(self.cfg.target_dir, output_file_name(spec["target"], self.current_time, ".npz")),
                     shape=np.array([self.rows, self.cols], np.int64), nodata=np.float64(frontend.NODATA),
                     select=np.array(spec["select"]), above=np.float64(spec["above"]), **entry)
        return entry

    # CModel::runModelOutputs (:870-891) + CDomainCartesian::writeOutputs (:804-829)
    def write_outputs(self):
        due = abs(self.current_time - self.last_output_time - self.output_frequency) < 1e-5 and \
            self.current_time > self.last_output_time
        if not due:
            return False
        self._state_now = None
        engines_own = lambda what: frontend.peak_value_code(what) is not None or what in ("infiltration", "tracer", "concentration", "deposit")
        derived = self._gather_plain([what for what, _ in self.cfg.targets if not engines_own(what)])
        overviews = self._gather_overviews()
        selection = self._gather_selection()
        self._state_now = None
        peaks = self.peaks()                                       # the peaks so far, written like maxdepth at every output time
        out = {}
        for k, (what, pattern) in enumerate(self.cfg.targets):
            arr, species = self._target_array(k, what, derived, peaks)
            out[what if species is None else (what, species)] = arr
            if species is not None and pattern:
                pattern = self._species_pattern(pattern, species)
            self._write_raster(pattern, arr, self.res, self.cfg.target_formats[k])
        for name, arr in peaks.items():                            # (asked for through Model(peaks=...) only: no file)
            out.setdefault(name, arr)
        for what, aggregate, factor, pattern, fmt in self.overview_list:
            out[(what, aggregate, factor)] = overviews[(what, aggregate, factor)]
            self._write_raster(pattern, out[(what, aggregate, factor)], factor * self.res, fmt)
        if selection is not None:
            out["sparse"] = self._write_selection(selection)
        self.write_probes()
        self.write_zones()
        self.write_links()
        self.write_outflow()
        self.outputs.append((self.current_time, out))
        self.last_output_time = self.current_time
        self.scheme.force_time_advance()
        if self.log:
            applies = f", {self.bed_applies} bed applies" if self.bed_shape_list else ""
            self.log(f"Output files written at {seconds_to_time(self.current_time)} ({len(out)} rasters{applies})")
        self.log_domain_stats()
        return True

    # CSchemeGodunov::prepareSimulation's "Initial domain volume" line (:1060) and the same figures at every output time
    def log_domain_stats(self, initial=False):
        if not hasattr(self.sim, "stats"):
            return None
        s = self.sim.stats()
        self.domain_stats.append((0.0 if initial else self.current_time, s))
        if self.log:
            if initial:
                self.log(f"Initial domain volume: {s['volume']:.0f} m3")
            else:
                self.log(f"Domain volume: {s['volume']:.0f} m3, wet cells: {s['cells_wet']} of {s['cells']}, "
                         f"max depth: {s['max_depth']:.3f} m, max speed: {s['max_speed']:.3f} m/s")
        return s

    # CModel::logProgress (:337-433): the same quantities; returned as a dict and, if a log sink is set, as a block
    def log_progress(self, seconds):
        t = min(self.current_time, self.simulation_time)
        progress = t / self.simulation_time if self.simulation_time > 0 else 1.0
        rate = int(self.scheme.cells_calculated / seconds) if seconds > 0 else 0
        remaining = min((1.0 - progress) * (seconds / progress), 31536000.0) if progress > 0 else 31536000.0
        block = dict(simulation_time=t, lowest_timestep=self.scheme.batch_timesteps, cells_calculated=self.scheme.cells_calculated,
                     rate=rate, processing_time=seconds, remaining=remaining, batch_size=self.scheme.queue_addition_size,
                     progress=progress)
        self.progress_blocks.append(block)
        if self.log:
            bar = "=" * max(0, int(math.floor(55 * progress)) - 1) + ">"
            self.log("\n".join([
                " SIMULATION PROGRESS",
                f" Simulation time:  {seconds_to_time(t):<15}Lowest timestep: {seconds_to_time(block['lowest_timestep']):>15}",
                f" Cells calculated: {block['cells_calculated']:<24}  Rate: {rate:>13}/s",
                f" Processing time:  {seconds_to_time(seconds):<16}Est. remaining: {seconds_to_time(remaining):>15}",
                f" Batch size:       {block['batch_size']:<16}",
                f" [{bar:<55}] {progress * 100:6.1f}%"]))
        return block

    # CModel::runModelMain (:1036-1100) for one local domain; the reference's polling of an asynchronous worker
    # collapses to a blocking batch per loop pass
    def run(self, max_outputs=None):
        t0 = self.clock()
        synchronised = True                                        # CModel.cpp:80: starts synchronised at t = 0
        while self.current_time < self.simulation_time - 1e-5:
            # runModelDomainAssess (:536-698)
            earliest = self.scheme.current_time
            sync_ready = self.scheme.is_sync_ready(self.target_time) and not synchronised and \
                self.last_sync_time != earliest
            synchronised = sync_ready
            self.current_time = earliest
            # runModelSync (:775-846): outputs, then a new target
            if synchronised or self.target_time == 0.0:
                self.last_sync_time = self.current_time
                self.write_outputs()
                if max_outputs is not None and len(self.outputs) >= max_outputs:
                    break
                self.update_target()
                synchronised = False
            # runModelSchedule (:905-957)
            self.scheme.run_simulation(self.target_time, self.clock() - t0)
            # runModelUI (:962-975)
            seconds = self.clock() - t0
            if seconds - self.last_progress > self.progress_interval:
                self.log_progress(seconds)
                self.last_progress = seconds
        # the loop ends once the last target is reached: one more assess + sync writes the final outputs
        self.current_time = self.scheme.current_time
        if self.scheme.is_sync_ready(self.target_time):
            self.write_outputs()
        self.write_probes()
        self.write_zones()
        self.seconds = self.clock() - t0
        self.log_progress(self.seconds)
        return self.outputs

    def close(self):
        if hasattr(self.sim, "close"):
            self.sim.close()
