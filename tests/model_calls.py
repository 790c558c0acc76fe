"""What Model says to its engine, and what it writes: a recording proxy around any engine object, the 40 x 32 model file that turns
every feature of hipims_mi.model.Model on at once, the oracle extended with inert stubs for the feature methods it lacks, and the
record of one run (the call log, the log lines, the output files with a hash of each).  tests/test_model_calls.py and
tests/test_gpu_model_calls.py compare such records against the ones the commit in front of the front end's split produced:

    python tests/model_calls.py cpu | gpu      writes tests/model_calls_expected.json | tests/model_calls_expected_gpu.json
"""
import hashlib
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
COLS, ROWS, DX = 40, 32, 2.0


# ---- the proxy -------------------------------------------------------------------------------------------------------------
def digest(v):
    """Arrays by shape, dtype and a hash of their bytes; scalars and strings as they are; lists, tuples and dicts recursively."""
    if isinstance(v, np.ndarray):
        return dict(shape=list(v.shape), dtype=str(v.dtype), sha1=hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest())
    if isinstance(v, np.generic):
        v = v.item()
    if isinstance(v, dict):
        return {str(k): digest(x) for k, x in sorted(v.items(), key=lambda kv: str(kv[0]))}
    if isinstance(v, (list, tuple)):
        return [digest(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return repr(v)                                                         # (JSON has no word for them)
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError(f"an engine argument of type {type(v).__name__}")


class Recorder:
    """Forwards everything to `engine`; every call of one of its methods is logged as [name, args, kwargs].  A name the engine
    lacks raises AttributeError here too, so hasattr answers as it does on the engine."""

    def __init__(self, engine):
        self.__dict__["engine"] = engine
        self.__dict__["calls"] = []

    def __getattr__(self, name):
        target = getattr(self.engine, name)
        if not callable(target):
            return target

        def logged(*args, **kwargs):
            self.calls.append([name, digest(args), digest(kwargs)])
            return target(*args, **kwargs)
        return logged

    def __setattr__(self, name, value):
        setattr(self.engine, name, value)


# ---- the model file --------------------------------------------------------------------------------------------------------
SOIL_CLASSES = [dict(ks=1e-5, suction=0.1, deficit=0.3), dict(ks=2e-6, suction=0.2, deficit=0.4, capacity=0.05)]
LINKS = [dict(a=(3, 3), b=(9, 3), kind=1, one_way=0, level=0.0, size=0.5, coeff=0.6, limit=np.inf)]
SOURCE_SILT = dict(cells=[(3, 5), (4, 5)], series=[(0.0, 1.0 / 3.0), (2.0, 1.0)])
SOURCE_DYE = dict(cells=[(4, 5), (30, 20)], series=[(0.0, 2.0)])

HEAD = """<?xml version="1.0"?>
<configuration><metadata><name>everything</name></metadata>
<simulation>
  <parameter name="duration" value="2.0"/><parameter name="outputFrequency" value="1.0"/>
  <domainSet><domain type="cartesian" deviceNumber="1">
    <data sourceDir="in" targetDir="out">
      <dataSource type="raster" value="structure,dem" source="dem.asc"/>
      <dataSource type="constant" value="depth" source="1.0"/>
      <dataSource type="constant" value="manningCoefficient" source="0.03"/>
      <dataSource type="raster" value="zones" source="zones.asc"/>
      <gauge name="pool" x="5" y="6"/>
      <section name="mid" x0="10" y0="4" x1="14" y1="20"/>
      <bedShape name="bank" mapFile="bank_cells.csv" source="bank_progress.csv"/>
      <dataTarget type="raster" value="depth" format="HFA" target="depth_%t.img"/>
      <dataTarget type="raster" value="velocityX" format="ASC" target="vx_%t.asc"/>
      <dataTarget type="raster" value="peakSpeed" format="ASC" target="peakspeed_%t.asc"/>
      <dataTarget type="raster" value="depth" overview="4" aggregate="max" format="ASC" target="depth_max4_%t.asc"/>
      <sparseTarget select="depth" above="1.0005" values="depth,velocityx" target="wet_%t.npz"/>
"""
SOIL = """      <dataSource type="raster" value="soil" source="soil.asc"/>
      <soilClasses source="soil.csv"/>
      <dataTarget type="raster" value="infiltration" format="ASC" target="soaked_%t.asc"/>
"""
TRACER_SET = """      <tracerSpecies name="silt" source="m0.asc" settling="0.001" tauDeposit="0.08" tauErode="0.25" erodibility="0.0002" deposit="d0.asc"/>
      <tracerSpecies name="dye" decay="0.25"/>
      <tracerSource species="silt" mapFile="cells_silt.csv" source="rate_silt.csv"/>
      <tracerSource species="dye" mapFile="cells_dye.csv" source="rate_dye.csv"/>
      <dataTarget type="raster" value="tracer" species="silt" format="ASC" target="tracer_%t.asc"/>
      <dataTarget type="raster" value="concentration" species="dye" format="ASC" target="conc_%s_%t.asc"/>
      <dataTarget type="raster" value="deposit" species="silt" format="ASC" target="deposit_%t.asc"/>
"""
TRACER_SINGLE = """      <dataSource type="raster" value="tracer" source="m0.asc"/>
      <tracerSource mapFile="cells_silt.csv" source="rate_silt.csv"/>
      <dataTarget type="raster" value="tracer" format="ASC" target="tracer_%t.asc"/>
      <dataTarget type="raster" value="concentration" format="ASC" target="conc_%t.asc"/>
"""
MIDDLE = """    </data>
    <scheme name="godunov"><parameter name="courantNumber" value="0.5"/></scheme>
    <boundaryConditions sourceDir="in">
      <domainEdge edge="north" treatment="closed"/><domainEdge edge="south" treatment="closed"/>
      <domainEdge edge="west" treatment="closed"/>
      <domainEdge edge="east" treatment="open" name="outlet" from="8" to="23"/>
      <timeseries type="atmospheric" name="rain" value="rain-intensity" source="rain.csv"/>
"""
LINK = """      <links mapFile="links.csv"/>
"""
TAIL = """    </boundaryConditions>
  </domain></domainSet>
</simulation></configuration>
"""


def write_model(tmp_path, links=True, soil=True, tracers="set"):
    """The model file and its inputs under tmp_path; `links`, `soil` and `tracers` ("set", "single" or None) leave features out
    (the HIP engine carries a tracer OR links and an infiltration: one file with them all it refuses)."""
    from hipims_mi import frontend
    src = os.path.join(str(tmp_path), "in")
    os.makedirs(src, exist_ok=True)
    y, x = np.mgrid[0:ROWS, 0:COLS]
    frontend.write_raster(os.path.join(src, "dem.asc"), np.round(0.002 * (COLS - x) + 0.001 * y, 4), DX)      # falls to the open east edge
    frontend.write_raster(os.path.join(src, "zones.asc"), np.where(x < 12, 1, np.where(y > 20, 2, 0)).astype(np.float64), DX)
    frontend.write_raster(os.path.join(src, "soil.asc"), np.where(x > 25, 2, np.where(y < 10, 0, 1)).astype(np.float64), DX)
    frontend.write_soil_csv(os.path.join(src, "soil.csv"), SOIL_CLASSES)
    frontend.write_links_csv(os.path.join(src, "links.csv"), LINKS)
    m0, d0 = np.zeros((ROWS, COLS)), np.zeros((ROWS, COLS))
    m0[5:8, 6:10] = 1.5
    d0[9:12, 3:20] = 0.25
    frontend.write_raster(os.path.join(src, "m0.asc"), m0, DX)
    frontend.write_raster(os.path.join(src, "d0.asc"), d0, DX)
    frontend.write_tracer_source_csv(os.path.join(src, "cells_silt.csv"), os.path.join(src, "rate_silt.csv"), SOURCE_SILT["cells"], SOURCE_SILT["series"])
    frontend.write_tracer_source_csv(os.path.join(src, "cells_dye.csv"), os.path.join(src, "rate_dye.csv"), SOURCE_DYE["cells"], SOURCE_DYE["series"])
    with open(os.path.join(src, "rain.csv"), "w") as f:
        f.write("time,rate\n0.0,36.0\n1.0,72.0\n2.0,36.0\n")
    with open(os.path.join(src, "bank_cells.csv"), "w") as f:
        f.write("x,y,target\n20,10,0.5\n21,10,0.5\n22,11,0.25\n")
    with open(os.path.join(src, "bank_progress.csv"), "w") as f:
        f.write("time,fraction\n0.0,0.0\n1.5,1.0\n")
    xml = os.path.join(str(tmp_path), "model.xml")
    with open(xml, "w") as f:
        f.write(HEAD + (SOIL if soil else "") + dict(set=TRACER_SET, single=TRACER_SINGLE).get(tracers, "") + MIDDLE + (LINK if links else "") + TAIL)
    return xml


# ---- the engines -----------------------------------------------------------------------------------------------------------
def host_sim_class():
    """The oracle with inert stubs for what acts inside an iteration: Model takes the host path for everything else."""
    import hipims_mi as hp
    import oracle

    class HostSim(oracle.OracleSim):
        def upload(self, state=None, bed=None, manning=None):
            if bed is not None:
                self.bed_now = np.array(bed, dtype=np.float64)
            super().upload(state, bed, manning)

        def stats(self):
            depth = np.maximum(self.download()[..., 0] - self.bed_now, 0.0) * (self.bed_now < 9999.0)
            return dict(volume=float(depth.sum() * self.dx * self.dx), cells_wet=int((depth > 1e-8).sum()), cells=int(depth.size),
                        max_depth=float(depth.max()), max_speed=0.0)

        def add_links(self, links):
            self.links = hp.pack_links(links, self.cols)

        def links_read(self):
            rec = np.zeros(len(self.links), hp.LINK_RECORD_DTYPE)
            rec["q_last"], rec["volume"] = 0.125, 1.0 / 3.0
            return rec

        def add_open(self, segments):
            self.segments = segments.copy()

        def open_read(self):
            rec = np.zeros(int((self.segments["last"] - self.segments["first"] + 1).sum()), hp.OPEN_RECORD_DTYPE)
            rec["q_last"], rec["volume"] = 1e-3 * (1 + np.arange(len(rec))), 0.1
            return rec

        def add_infiltration(self, soil, classes, initial=None):
            self.soaked = 0.001 * np.asarray(soil, dtype=np.float64)

        def infiltration_read(self, row0=0, nrows=None):
            return self.soaked.copy()

        def tracer_enable(self, initial=None):
            self.m = np.zeros((1, self.rows, self.cols)) if initial is None else np.array(initial, dtype=np.float64)[None]

        def tracer_enable_set(self, initial=None, decay=None, species=None):
            self.m = np.array(initial, dtype=np.float64)
            self.d = np.zeros_like(self.m)

        def tracer_add_source(self, cells, series, species=0):
            pass

        def tracer_read(self, row0=0, nrows=None, species=0):
            return self.m[species].copy()

        def tracer_set_exchange(self, species, settling=0.0, tau_deposit=np.inf, tau_erode=np.inf, erodibility=0.0, deposit=None):
            if deposit is not None:
                self.d[species] = deposit

        def tracer_deposit_read(self, species=0, row0=0, nrows=None):
            return self.d[species].copy()
    return HostSim


def device_sim_class():
    """... and with derive, peaks_*, probes_*, zones_*, overview, sparse and bed_* on top, each the front end's own host class behind
    the engine's name: Model takes the device path everywhere."""
    from hipims_mi import frontend

    class DeviceSim(host_sim_class()):
        def _t(self):
            return self.scalars()["t"]

        def download(self, which=0):
            return self.bed_now.copy() if which == 1 else super().download()

        def derive(self, values, **kw):
            state = self.download()
            return {v: frontend.derive_output(v, state, self.bed_now, self.dx) for v in values}

        def overview(self, values, aggregates, factor, **kw):
            state = self.download()
            return [frontend.overview(frontend.derive_output(v, state, self.bed_now, self.dx), factor, a) for v, a in zip(values, aggregates)]

        def sparse(self, values, select="depth", above=0.0, **kw):
            state = self.download()
            return frontend.sparse([frontend.derive_output(v, state, self.bed_now, self.dx) for v in values],
                                   frontend.derive_output(select, state, self.bed_now, self.dx), above)

        def peaks_enable(self, values, arrival_depth=0.01):
            self.peak_tracker = frontend.PeakTracker(self.rows, self.cols, arrival_depth, t=self._t())

        def peaks_sample(self):
            self.peak_tracker.fold(self.download(), self.bed_now, self._t())

        def peaks(self, values):
            return {v: self.peak_tracker.rasters()[v] for v in values}

        def probes_enable(self, gauges=(), sections=(), capacity=4096):
            self.probe_recorder = frontend.ProbeRecorder(gauges, sections, self.dx)

        def probes_sample(self):
            self.probe_recorder.record(self.download(), self.bed_now, self._t())

        def probes(self):
            return self.probe_recorder.series()

        def zones_enable(self, ids, zone_count=None, flood_depth=0.1, capacity=4096):
            self.zone_recorder = frontend.ZoneRecorder(ids, zone_count, flood_depth, self.dx)

        def zones_sample(self):
            self.zone_recorder.record(self.download(), self.bed_now, self._t())

        def zones(self):
            return self.zone_recorder.series()

        def bed_shape_add(self, cells, target, series):
            self.bed_shapes = getattr(self, "bed_shapes", None) or frontend.BedShapes(self.rows, self.cols)
            self.bed_shapes.add(cells, target, series, bed=self.bed_now)

        def bed_apply(self):
            state = np.ascontiguousarray(self.download())
            self.bed_shapes.apply(state, self.bed_now, self._t())
            super().upload(state, self.bed_now)
    return DeviceSim


def oracle_engine(cls):
    return lambda cfg, cols, rows, res: Recorder(cls(cols, rows, dx=res, scheme=cfg.scheme, precision=cfg.precision, very_small=cfg.dry_threshold,
                                                     courant=cfg.courant, end_time=cfg.duration, friction=cfg.friction))


def hip_engine(cfg, cols, rows, res):
    """The Domain that Model makes for itself, inside the proxy."""
    import hipims_mi as hp
    return Recorder(hp.Domain(cols, rows, dx=res, scheme=cfg.scheme, precision=cfg.precision, dry_threshold=cfg.dry_threshold, courant=cfg.courant,
                              t_end=cfg.duration, dynamic_dt=cfg.dynamic_dt, dt_fixed=cfg.timestep, dt_initial=cfg.timestep, friction=cfg.friction,
                              device=cfg.device_number - 1))


# ---- one run ---------------------------------------------------------------------------------------------------------------
def file_digest(path):
    """A hash of the file's bytes; of an .npz (a zip archive: it carries the time it was written) its arrays' digests instead."""
    if path.endswith(".npz"):
        with np.load(path) as z:
            return {k: digest(z[k]) for k in sorted(z.files)}
    with open(path, "rb") as f:
        return hashlib.sha1(f.read()).hexdigest()


def run_case(tmp_path, make_sim, output_format, hash_files=True, batch=3, **model_file):
    """Build the Model of write_model(tmp_path, **model_file) over make_sim's engine and run it with a fixed batch size.  -> the record:
    calls, log lines (without the progress blocks, which quote the wall clock), files {name: digest}; a refusal by the engine ends the
    record with its error."""
    from hipims_mi.model import Model
    xml = write_model(tmp_path, **model_file)
    engines, lines = [], []

    def make(*a):
        engines.append(make_sim(*a))
        return engines[0]
    record = {}
    try:
        m = Model(xml, make_sim=make, output_format=output_format, log=lines.append, peaks=["hazard"], gauges={"far": (30, 25)},
                  overviews=[("fsl", "min", 8)])
        try:
            m.scheme.automatic_queue = False
            m.scheme.queue_addition_size = batch
            m.run()
        finally:
            m.close()
    except (RuntimeError, NotImplementedError) as e:
        record["error"] = f"{type(e).__name__}: {e}"
        if engines and hasattr(engines[0], "close"):
            engines[0].engine.close()
    out = os.path.join(str(tmp_path), "out")
    names = sorted(os.listdir(out)) if os.path.isdir(out) else []
    record.update(calls=engines[0].calls if engines else [], log=[l for l in lines if "SIMULATION PROGRESS" not in l],
                  files={n: file_digest(os.path.join(out, n)) if hash_files else None for n in names})
    return json.loads(json.dumps(record))


CPU_CASES = dict(host=dict(sim="host", output_format="xml"), device=dict(sim="device", output_format=".npy"),
                 single=dict(sim="host", output_format=".npy", tracers="single"))
# the HIP engine refuses a tracer beside links or an infiltration: the whole file up to that refusal, then one file per side
GPU_CASES = dict(everything=dict(), water=dict(tracers=None), tracers=dict(links=False, soil=False), single=dict(links=False, soil=False, tracers="single"))


def cpu_records(tmp_path):
    sims = dict(host=host_sim_class(), device=device_sim_class())
    return {name: run_case(os.path.join(str(tmp_path), name), oracle_engine(sims[c["sim"]]), c["output_format"], tracers=c.get("tracers", "set"))
            for name, c in CPU_CASES.items()}


def gpu_records(tmp_path):
    """On the GPU the rasters' bytes are the kernels' business (tests/test_gpu_*.py pin them): the files are listed, not hashed."""
    return {name: run_case(os.path.join(str(tmp_path), name), hip_engine, ".npy", hash_files=False, **c) for name, c in GPU_CASES.items()}


if __name__ == "__main__":
    import tempfile
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "hipims-ocl_amd")):
        sys.path.insert(0, p)
    which = sys.argv[1] if len(sys.argv) > 1 else "cpu"
    target = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "model_calls_expected.json" if which == "cpu" else "model_calls_expected_gpu.json")
    with tempfile.TemporaryDirectory() as tmp:
        records = cpu_records(tmp) if which == "cpu" else gpu_records(tmp)
    with open(target, "w") as f:
        json.dump(records, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{target}: " + ", ".join(f"{name}: {len(r['calls'])} calls, {len(r['files'])} files" + (", refused" if "error" in r else "") for name, r in records.items()))
