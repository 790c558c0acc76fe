"""Front end for HiPIMS model directories: read the XML configuration, the CSV boundary series
and the rasters it names, run the model on the HIP engine at the reference's output times and write the reference's
output rasters -- without GDAL / boost / TinyXML.

What is mirrored (paths relative to the reference's src/):
  * configuration walk          Datasets/CXMLDataset.cpp:115-265, CModel.cpp:65-129 (duration, outputFrequency,
                                floatingPointPrecision), Schemes/CSchemeGodunov.cpp:128-333 + CScheme.cpp:60-135
                                (scheme parameters), Boundaries/CBoundaryMap.cpp:104-190 (timeseries elements)
  * initial conditions          Domain/Cartesian/CDomainCartesian.cpp:163-283 (DEM, then depth/FSL, then the rest),
                                CDomain.cpp:294-397 (4-decimal rounding of every input, quirk Q10), raster rows flipped
                                south-up (Datasets/CRasterDataset.cpp:411)
  * CSV series                  Boundaries/CBoundaryUniform.cpp:103-170 (header skipped, interval = t1 - t0,
                                length = last time), CBoundaryCell.cpp:164-300
  * main loop                   CModel.cpp:723-770, :870-891 (sync at every output time), CSchemeGodunov::runSimulation
  * output derivations          Datasets/CRasterDataset.cpp:185-267 (depth, velocity, fsl, maxdepth, maxfsl, froude;
                                threshold 1e-8, NODATA -9999)
Rasters: HFA .img through hipims_mi.hfa, ESRI ASCII .asc and NumPy .npy (read and write).
<domainEdge treatment="closed"> is honoured (bed = 9999.9 on that edge, CDomainCartesian.cpp:773-799); the reference
never parses the element (quirk Q9), so its own behaviour there is undefined.
"""
from __future__ import annotations

import csv
import math
import os
import xml.etree.ElementTree as ET
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np

from . import (DEPTH_IGNORE, DEPTH_IS_DEPTH, DEPTH_IS_FSL, DISCHARGE_IGNORE, DISCHARGE_IS_DISCHARGE,
               DISCHARGE_IS_VELOCITY, DISCHARGE_IS_VOLUME, SCHEME_GODUNOV, SCHEME_INERTIAL, SCHEME_MUSCL_HANCOCK,
               UNIFORM_LOSS_RATE,
               UNIFORM_RAIN_INTENSITY, ZONE_WORDS, ZONES_MAX, hfa, split_zone_records)

NODATA = -9999.0


def util_round(values, places=4):
    """Util::round (util.cpp:69-82): scale, then ceil if the fractional part (C fmod, sign of the dividend) is >= 0.5
    else floor -- so negative values round towards minus infinity unless they are integers."""
    v = np.asarray(values, dtype=np.float64) * (10 ** places)
    rem = np.fmod(v, 1.0)
    return np.where(rem >= 0.5, np.ceil(v), np.floor(v)) / (10 ** places)


# ------------------------------------------------------------------------------------------------ rasters
def read_raster(path):
    """-> (array[rows, cols] with row 0 = SOUTH, info{cols, rows, pixel_size?})"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".img":
        return hfa.read_raster(path)
    if ext == ".npy":
        a = np.load(path).astype(np.float64)
        return a, dict(cols=a.shape[1], rows=a.shape[0])
    if ext == ".asc":
        hdr = {}
        with open(path) as f:
            for _ in range(6):
                k, v = f.readline().split()
                hdr[k.lower()] = float(v)
            a = np.loadtxt(f, dtype=np.float64)
        nod = hdr.get("nodata_value", NODATA)
        a = np.where(a == nod, NODATA, a)
        return np.ascontiguousarray(a[::-1]), dict(cols=int(hdr["ncols"]), rows=int(hdr["nrows"]),
                                                   pixel_size=(hdr["cellsize"], hdr["cellsize"]))
    raise ValueError(f"unsupported raster format: {path}")


def write_raster(path, south_up, resolution, origin=(0.0, 0.0)):
    ext = os.path.splitext(path)[1].lower()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if ext == ".npy":
        np.save(path, south_up)
    elif ext == ".img":                        # format="HFA" in the reference's XML (CDomainCartesian.cpp:300, CRasterDataset.cpp:101-183)
        hfa.write_raster(path, south_up, resolution, origin)
    elif ext == ".asc":
        with open(path, "w") as f:
            f.write(f"ncols {south_up.shape[1]}\nnrows {south_up.shape[0]}\nxllcorner {origin[0]}\nyllcorner {origin[1]}\n"
                    f"cellsize {resolution}\nNODATA_value {NODATA}\n")
            np.savetxt(f, south_up[::-1], fmt="%.10g")
    else:
        raise ValueError(f"unsupported output format: {path}")


# ------------------------------------------------------------------------------------------------ configuration
@dataclass
class Boundary:
    kind: str                 # "atmospheric" (uniform) | "cell"
    name: str
    value: str                # rain-intensity | loss-rate ; for cell: depthValue/dischargeValue pair
    series: np.ndarray        # [n, 2] or [n, 4]
    depth_value: str = "fsl"
    discharge_value: str = "total"
    cells: list = field(default_factory=list)      # (x, y) for cell boundaries


@dataclass
class Configuration:
    name: str = ""
    duration: float = 0.0
    output_frequency: float = 0.0
    precision: str = "f64"
    scheme: int = SCHEME_GODUNOV
    courant: float = 0.5
    dry_threshold: float = 1e-10
    friction: bool = True
    dynamic_dt: bool = True
    timestep: float = 0.001
    source_dir: str = ""
    target_dir: str = ""
    sources: list = field(default_factory=list)    # (type, value-list, source)
    targets: list = field(default_factory=list)    # (value, target pattern)
    closed_edges: set = field(default_factory=set)
    boundaries: list = field(default_factory=list)
    device_number: int = 1
    gauges: list = field(default_factory=list)     # (name, x, y): <gauge> elements, cell indices (no reference counterpart)
    sections: list = field(default_factory=list)   # (name, x0, y0, x1, y1): <section> elements, cell indices
    overviews: list = field(default_factory=list)  # (value, aggregate, factor, target pattern, format): <dataTarget overview="...">
    sparse: dict = None                            # select, above, values, target pattern: the <sparseTarget> element (the last one wins)
    bed_shapes: list = field(default_factory=list)  # dict(name, cells [(x, y)], target [n], series [m, 2]): <bedShape> elements
    links: list = field(default_factory=list)      # dict(a (x, y), b (x, y), kind, one_way, level, size, coeff, limit): rows of the <links> elements' mapFiles
    soil_classes: list = field(default_factory=list)  # dict(ks, suction, deficit, capacity): rows of the <soilClasses> element's source; the id raster is the "soil" data source
    open_edges: list = field(default_factory=list)  # dict(edge, name, first, last): <domainEdge treatment="open"> elements; first / last None = the whole edge
    tracer_sources: list = field(default_factory=list)  # dict(cells [(x, y)], series [m, 2], species name or None): <tracerSource> elements; the initial M is the "tracer" data source
    tracer_species: list = field(default_factory=list)  # dict(name, decay, initial file or None[, exchange dict, deposit file or None]): <tracerSpecies> elements, the species of a tracer set
    target_species: list = field(default_factory=list)  # per entry of `targets`: the species="..." of a tracer / concentration target, or None
    target_formats: list = field(default_factory=list)  # per entry of `targets`: the GDAL driver name of its format="..." attribute, upper case (CDomainCartesian.cpp:300)


def _params(elem):
    return {p.get("name").lower(): p.get("value") for p in elem.findall("parameter")}


def _read_csv(path):
    rows = []
    with open(path, newline="") as f:
        for i, row in enumerate(csv.reader(f)):
            if i == 0 or not row or all(not c.strip() for c in row):      # header skipped unconditionally (:103-110)
                continue
            rows.append([float(c) for c in row])
    return np.array(rows, np.float64)


def parse_configuration(xml_path):
    """Datasets/CXMLDataset.cpp:115-265 for the single-domain Cartesian case."""
    base = os.path.dirname(os.path.abspath(xml_path))
    root = ET.parse(xml_path).getroot()
    cfg = Configuration()
    meta = root.find("metadata")
    if meta is not None and meta.find("name") is not None:
        cfg.name = meta.find("name").text or ""
    sim = root.find("simulation")
    sp = _params(sim)
    cfg.duration = float(sp.get("duration", 0))                               # CModel.cpp:78-129
    cfg.output_frequency = float(sp.get("outputfrequency", cfg.duration))
    cfg.precision = "f32" if sp.get("floatingpointprecision", "double").lower() == "single" else "f64"
    dom = sim.find("domainSet").find("domain")
    if (dom.get("type") or "cartesian").lower() != "cartesian":
        raise ValueError("only cartesian domains")
    cfg.device_number = int(dom.get("deviceNumber") or 1)
    data = dom.find("data")
    cfg.source_dir = os.path.join(base, data.get("sourceDir") or "")
    cfg.target_dir = os.path.join(base, data.get("targetDir") or "")
    for ds in data.findall("dataSource"):
        cfg.sources.append(((ds.get("type") or "").lower(), [v.strip().lower() for v in (ds.get("value") or "").split(",")],
                            ds.get("source")))
    for dt in data.findall("dataTarget"):
        if dt.get("overview") is not None:   # a block-aggregated overview of the value (no reference counterpart): not a full raster
            cfg.overviews.append(((dt.get("value") or "").lower(), aggregate_name(dt.get("aggregate") or "max"), int(dt.get("overview")),
                                  dt.get("target"), (dt.get("format") or "").upper()))
            continue
        cfg.targets.append(((dt.get("value") or "").lower(), dt.get("target")))
        cfg.target_species.append(dt.get("species"))
        cfg.target_formats.append((dt.get("format") or "").upper())
    for sp in data.findall("sparseTarget"):   # the values at the selected cells only, as CSR in one .npz (no reference counterpart)
        cfg.sparse = dict(select=(sp.get("select") or "depth").lower(), above=float(sp.get("above") or 0.0),
                          values=[v.strip().lower() for v in (sp.get("values") or sp.get("select") or "depth").split(",") if v.strip()],
                          target=sp.get("target"))
    # the probe recorder's elements (no reference counterpart): cell indices, the convention of a cell boundary's mapFile
    for k, g in enumerate(data.findall("gauge")):
        cfg.gauges.append((g.get("name") or f"gauge{k}", int(g.get("x")), int(g.get("y"))))
    for k, e in enumerate(data.findall("section")):
        cfg.sections.append((e.get("name") or f"section{k}", int(e.get("x0")), int(e.get("y0")), int(e.get("x1")), int(e.get("y1"))))
    # the moving bed's elements (no reference counterpart): mapFile rows are x, y, target elevation; source rows time, fraction
    for k, e in enumerate(data.findall("bedShape")):
        cells = _read_csv(os.path.join(cfg.source_dir, e.get("mapFile"))).reshape(-1, 3)
        series = _read_csv(os.path.join(cfg.source_dir, e.get("source"))).reshape(-1, 2)
        cfg.bed_shapes.append(dict(name=e.get("name") or f"bedShape{k}", cells=[(int(r[0]), int(r[1])) for r in cells],
                                   target=cells[:, 2].copy(), series=series))
    # the infiltration's classes (no reference counterpart): <soilClasses source="soil.csv"/>, rows ks, suction, deficit, capacity ("inf" is
    # a number to float()); class k of the raster <dataSource type="raster" value="soil" source="..."/> is row k
    for e in data.findall("soilClasses"):
        cfg.soil_classes = [dict(ks=float(r[0]), suction=float(r[1]), deficit=float(r[2]), capacity=float(r[3]))
                            for r in _read_csv(os.path.join(cfg.source_dir, e.get("source"))).reshape(-1, 4)]
    # the tracer's sources (no reference counterpart): <tracerSource mapFile="cells.csv" source="rate.csv"/>, mapFile rows x, y; source rows
    # time, mass rate.  The initial M is the raster <dataSource type="raster" value="tracer" source="m0.asc"/>
    for e in data.findall("tracerSource"):
        cells = _read_csv(os.path.join(cfg.source_dir, e.get("mapFile"))).reshape(-1, 2)
        cfg.tracer_sources.append(dict(cells=[(int(r[0]), int(r[1])) for r in cells],
                                       series=_read_csv(os.path.join(cfg.source_dir, e.get("source"))).reshape(-1, 2), species=e.get("species")))
    # a tracer set's species: <tracerSpecies name="sewage" decay="2.3e-5" source="m0.asc"/> (decay in 1/s, default 0; source: the initial M, a
    # raster, default zeros); <tracerSource species="sewage" .../> feeds it, <dataTarget value="tracer|concentration" species="sewage" .../> writes it
    # ... and what it exchanges with the bed: settling= (m/s) tauDeposit= tauErode= (N/m2) erodibility= (units/(m2 s)) deposit= (the initial
    # deposit D, a raster); any of them makes the species one that exchanges; <dataTarget value="deposit" species="silt" .../> writes D
    for k, e in enumerate(data.findall("tracerSpecies")):
        said = {name: float(e.get(attr)) for name, attr in (("settling", "settling"), ("tau_deposit", "tauDeposit"), ("tau_erode", "tauErode"),
                                                            ("erodibility", "erodibility")) if e.get(attr) is not None}
        cfg.tracer_species.append(dict(name=e.get("name") or f"species{k}", decay=float(e.get("decay") or 0.0), initial=e.get("source")))
        if said or e.get("deposit"):                                           # (a species without them keeps the three keys it had)
            cfg.tracer_species[-1].update(exchange=said, deposit=e.get("deposit"))
    sch = dom.find("scheme")
    name = (sch.get("name") or "godunov").lower()
    # CScheme::createFromConfig (CScheme.cpp:140-176): "muscl-hancock" | "godunov" | "inertial"
    cfg.scheme = {"muscl-hancock": SCHEME_MUSCL_HANCOCK, "muscl": SCHEME_MUSCL_HANCOCK,
                  "inertial": SCHEME_INERTIAL}.get(name, SCHEME_GODUNOV)
    sp = _params(sch)
    cfg.courant = float(sp.get("courantnumber", 0.5))                         # CSchemeGodunov.cpp:128-333
    cfg.dry_threshold = float(sp.get("drythreshold", 1e-10))
    cfg.friction = sp.get("frictioneffects", "yes").lower() in ("yes", "true", "1")
    if sp.get("timestepmode", "cfl").lower() == "fixed":
        cfg.dynamic_dt = False
    cfg.timestep = float(sp.get("timestepinitial", sp.get("timestepfixed", 0.001)))
    bc = dom.find("boundaryConditions")
    if bc is not None:
        bdir = os.path.join(base, bc.get("sourceDir") or "")
        for e in bc.findall("domainEdge"):
            if (e.get("treatment") or "").lower() == "closed":
                cfg.closed_edges.add((e.get("edge") or "").lower())
            # the open boundary (no reference counterpart): <domainEdge edge="east" treatment="open" name="outlet" from="8" to="23"/>,
            # from / to: indices along the edge, inclusive; without them the whole edge (its corners excepted)
            elif (e.get("treatment") or "").lower() == "open":
                edge = (e.get("edge") or "").lower()
                if edge not in ("north", "south", "east", "west"):
                    raise ValueError(f"unknown domainEdge {edge!r}")
                cfg.open_edges.append(dict(edge=edge, name=e.get("name") or f"{edge}{len(cfg.open_edges)}",
                                           first=None if e.get("from") is None else int(e.get("from")),
                                           last=None if e.get("to") is None else int(e.get("to"))))
        for ts in bc.findall("timeseries"):
            kind = (ts.get("type") or "").lower()
            series = _read_csv(os.path.join(bdir, ts.get("source")))
            b = Boundary(kind=kind, name=ts.get("name") or "", value=(ts.get("value") or "rain-intensity").lower(),
                         series=series, depth_value=(ts.get("depthValue") or "fsl").lower(),
                         discharge_value=(ts.get("dischargeValue") or "total").lower())
            if kind == "cell" and ts.get("mapFile"):
                b.cells = [(int(r[0]), int(r[1])) for r in _read_csv(os.path.join(bdir, ts.get("mapFile")))]
            cfg.boundaries.append(b)
        # link groups (no reference counterpart): <links mapFile="links.csv"/>, rows xa, ya, xb, yb, kind, one_way, level, size, coeff, limit
        # (kind: 0 weir, 1 orifice, 2 pump; "inf" is a number to float())
        for e in bc.findall("links"):
            for r in _read_csv(os.path.join(bdir, e.get("mapFile"))).reshape(-1, 10):
                cfg.links.append(dict(a=(int(r[0]), int(r[1])), b=(int(r[2]), int(r[3])), kind=int(r[4]), one_way=int(r[5]),
                                      level=float(r[6]), size=float(r[7]), coeff=float(r[8]), limit=float(r[9])))
    return cfg


def write_links_csv(path, links):
    """The mapFile of a <links> element: what parse_configuration reads back (repr round-trips every double)."""
    with open(path, "w") as f:
        f.write("xa,ya,xb,yb,kind,one_way,level,size,coeff,limit\n")
        for l in links:
            f.write(",".join([str(int(l["a"][0])), str(int(l["a"][1])), str(int(l["b"][0])), str(int(l["b"][1])), str(int(l["kind"])),
                              str(int(l.get("one_way", 0)))] + [repr(float(l[k])) for k in ("level", "size", "coeff", "limit")]) + "\n")


# ------------------------------------------------------------------------------------------------ domain arrays
def build_domain(cfg):
    """loadInitialConditions order: DEM, depth/FSL, everything else (CDomainCartesian.cpp:163-283)."""
    structure = next((s for s in cfg.sources if "structure" in s[1]), None) or next(s for s in cfg.sources if "dem" in s[1])
    ref, info = read_raster(os.path.join(cfg.source_dir, structure[2]))
    rows, cols = ref.shape
    res = float(info.get("pixel_size", (1.0, 1.0))[0])
    bed = np.zeros((rows, cols))
    state = np.zeros((rows, cols, 4))
    man = np.zeros((rows, cols))

    def values(src):
        if src[0] == "constant":
            return np.full((rows, cols), float(src[2]))
        return read_raster(os.path.join(cfg.source_dir, src[2]))[0]

    ordered = sorted(cfg.sources, key=lambda s: 0 if "dem" in s[1] else (1 if ({"depth", "fsl"} & set(s[1])) else 2))
    for src in ordered:
        v = None
        for what in src[1]:
            if what == "structure":
                continue
            v = values(src) if v is None else v
            if what == "dem":
                bed[...] = util_round(v); state[..., 0] = bed                     # CDomain.cpp:304-316
            elif what == "fsl":
                state[..., 0] = util_round(v); state[..., 1] = state[..., 0]
            elif what == "depth":
                state[..., 0] = util_round(bed + v); state[..., 1] = state[..., 0]
            elif what == "disabled":
                state[..., 1] = np.where((v > 1.0) & (v < 9999.0), -9999.0, state[..., 1])
            elif what == "dischargex":
                state[..., 2] = util_round(v)
            elif what == "dischargey":
                state[..., 3] = util_round(v)
            elif what == "velocityx":
                state[..., 2] = util_round(v * (state[..., 0] - bed))
            elif what == "velocityy":
                state[..., 3] = util_round(v * (state[..., 0] - bed))
            elif what == "manningcoefficient":
                man[...] = util_round(v)
    for edge in cfg.closed_edges:                                                 # CDomainCartesian.cpp:773-799
        sl = {"north": np.s_[-1, :], "south": np.s_[0, :], "east": np.s_[:, -1], "west": np.s_[:, 0]}[edge]
        bed[sl] = 9999.9
    return state, bed, man, res


def _cell_codes(b):
    depth = {"fsl": DEPTH_IS_FSL, "depth": DEPTH_IS_DEPTH, "ignore": DEPTH_IGNORE, "disabled": DEPTH_IGNORE}[b.depth_value]
    disc = {"total": DISCHARGE_IS_DISCHARGE, "cell": DISCHARGE_IS_DISCHARGE, "velocity": DISCHARGE_IS_VELOCITY,
            "ignore": DISCHARGE_IGNORE, "disabled": DISCHARGE_IGNORE, "volume": DISCHARGE_IS_VOLUME,
            "surging": DISCHARGE_IS_VOLUME}[b.discharge_value]
    return depth, disc


def attach_boundaries(cfg, sim, cols):
    """Works for hipims_mi.Domain and for the oracle's simulation objects (same add_* surface)."""
    for b in cfg.boundaries:
        s = b.series
        if b.kind == "atmospheric":
            interval, length = s[1, 0] - s[0, 0], s[-1, 0]                          # CBoundaryUniform.cpp:156-160
            definition = UNIFORM_LOSS_RATE if b.value == "loss-rate" else UNIFORM_RAIN_INTENSITY
            sim.add_uniform(definition, s[:, :2], interval, length)
        elif b.kind == "cell":
            depth, disc = _cell_codes(b)
            ser = s[:, :4].copy()
            if b.discharge_value == "total":                                        # CBoundaryCell.cpp:398-402
                ser[:, 2:4] /= max(1, len(b.cells))
            sim.add_cell(depth, disc, [y * cols + x for x, y in b.cells], ser, s[1, 0] - s[0, 0], s[-1, 0])
        else:
            raise ValueError(f"unsupported timeseries type {b.kind}")


# ------------------------------------------------------------------------------------------------ outputs
def data_value_code(name):
    """CDomain::getDataValueCode (CDomain.cpp:464-500): SUBSTRING matches, in the reference's order (so "maxdepth"
    wins over "depth", "maxfsl" over "fsl")."""
    n = (name or "").lower()
    if "dem" in n:
        return "dem"
    if "maxdepth" in n:
        return "maxdepth"
    if "depth" in n:
        return "depth"
    for key in ("disabled", "dischargex", "dischargey"):
        if key in n:
            return key
    if "maxfsl" in n:
        return "maxfsl"
    if "fsl" in n:
        return "fsl"
    for key in ("manningcoefficient", "velocityx", "velocityy", "froude"):
        if key in n:
            return key
    return None


PEAK_NAMES = ("peakspeed", "peakunitdischarge", "hazard", "arrivaltime", "wetduration")     # = hipims_mi.PEAK_CODES, in code order


def peak_value_code(name):
    """The peak tracker's value names (no reference counterpart): exact matches, case-insensitive.  None of them contains a
    substring data_value_code matches, so a <dataTarget> is either an output raster or a peak, never both."""
    n = (name or "").strip().lower()
    return n if n in PEAK_NAMES else None


class PeakTracker:
    """The peak tracker in NumPy, in exactly the device kernel's operation order (csrc/hp_peaks.hpp: track_peaks): the
    reference the GPU tests compare against bit for bit, and the tracker of engines without the device path.  All arithmetic
    in fp64; only add, multiply, divide, sqrt and compare.

        reset(t)               NODATA everywhere, t_previous = t
        fold(state, bed, t)    one sample: state[rows, cols, 4] = {Z, Zmax, Qx, Qy}, bed[rows, cols], t = the model time
        rasters()              {name: array} of the five values so far
    """

    def __init__(self, rows, cols, arrival_depth=0.01, t=0.0):
        if not arrival_depth >= 1e-8:
            raise ValueError("arrival_depth must be at least 1e-8")
        self.shape, self.arrival_depth = (int(rows), int(cols)), float(arrival_depth)
        self.reset(t)

    def reset(self, t):
        self.acc = {name: np.full(self.shape, NODATA) for name in PEAK_NAMES}
        self.t_previous = self.t_first = self.t_last = float(t)
        self.samples = 0

    def fold(self, state, bed, t):
        z, zmax, qx, qy = (state[..., k].astype(np.float64) for k in range(4))
        zb = np.asarray(bed).astype(np.float64)
        t = float(t)
        with np.errstate(all="ignore"):                                       # (cells that are not hit may hold anything)
            self._fold(z, zmax, qx, qy, zb, t)
        if self.samples == 0:
            self.t_first = t
        self.t_previous = self.t_last = t
        self.samples += 1

    def _fold(self, z, zmax, qx, qy, zb, t):
        depth = z - zb
        hit = (zmax > -9999.0) & (zb <= 9999.0) & (depth > 1e-8)             # counted (domain_stats) and wet (the output stage)
        div = np.where(hit, depth, 1.0)                                       # (a dry cell's quotient is never formed)
        vx, vy = qx / div, qy / div
        v = np.sqrt(vx * vx + vy * vy)
        for name, value in (("peakspeed", v), ("peakunitdischarge", np.sqrt(qx * qx + qy * qy)), ("hazard", depth * (v + 0.5))):
            a = self.acc[name]
            larger = hit & (value > a)
            a[larger] = value[larger]
        over = hit & (depth > self.arrival_depth)
        a = self.acc["arrivaltime"]
        a[over & (a == NODATA)] = t
        a = self.acc["wetduration"]
        a[over] = np.where(a[over] == NODATA, 0.0, a[over]) + (t - self.t_previous)

    def rasters(self):
        return {name: a.copy() for name, a in self.acc.items()}

    def info(self):
        return dict(samples=self.samples, t_first=self.t_first, t_last=self.t_last)


# ------------------------------------------------------------------------------------------------ probes (gauges and sections)
class Section(NamedTuple):
    """A cross-section: cells[m, 2] as (x, y) cell indices and one weight pair in {-1, 0, 1} per cell.  Its discharge is
    dx * sum(wx * Qx + wy * Qy) over its counted, wet cells."""
    cells: np.ndarray
    wx: np.ndarray
    wy: np.ndarray


def rasterise_section(p0, p1):
    """The cells of the straight cross-section from cell p0 = (x0, y0) to cell p1 = (x1, y1): a monotone, 4-connected path of
    exactly |x1 - x0| + |y1 - y0| + 1 cells.  At every cell the next step is the one (along x or along y) that ends nearer the
    straight line -- integer arithmetic on the cross product, a tie goes to x --, which keeps every cell centre within
    (|dx| + |dy|) / (2 hypot(dx, dy)) <= 0.71 cell widths of the segment.  A step from cell k to cell k + 1 with direction
    (tx, ty) belongs to cell k and carries the left normal (wx, wy) = (-ty, tx); the last cell carries (0, 0).  So the discharge is
    positive when water crosses from the right of the direction of travel to its left, and for a uniform wet field Q = (a, b) it
    is dx * (b * (x1 - x0) - a * (y1 - y0))."""
    (x0, y0), (x1, y1) = (int(p0[0]), int(p0[1])), (int(p1[0]), int(p1[1]))
    ax, ay = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x1 > x0 else -1), (1 if y1 > y0 else -1)
    cells, wx, wy = [(x0, y0)], [], []
    i = j = 0                                   # steps taken along x and along y
    e = 0                                       # i * ay - j * ax: (ax, ay) x the offset from the line, in cell widths x hypot
    while i < ax or j < ay:
        along_x = j == ay or (i < ax and abs(e + ay) <= abs(e - ax))
        if along_x:
            i, e = i + 1, e + ay
            wx.append(0); wy.append(sx)
        else:
            j, e = j + 1, e - ax
            wx.append(-sy); wy.append(0)
        cells.append((x0 + sx * i, y0 + sy * j))
    wx.append(0); wy.append(0)
    return Section(np.array(cells, np.int64).reshape(-1, 2), np.array(wx, np.int8), np.array(wy, np.int8))


def fold_section_terms(terms, dx):
    """A section's discharge from its terms, in exactly record_probes' order (csrc/hp_probes.hpp): 256 partial sums, partial j =
    +0.0 + term[j] + term[j + 256] + ... in that order, folded by the halving tree part[i] = part[i] + part[i + s] for s = 128,
    ..., 1, then dx * part[0].  (The list is padded with +0.0 to whole rows of 256: a partial sum that starts from +0.0 is never
    -0.0, so adding +0.0 to it changes no bit.)"""
    terms = np.asarray(terms, dtype=np.float64).reshape(-1)
    rows = -(-terms.size // 256)
    padded = np.zeros(rows * 256)
    padded[:terms.size] = terms
    part = np.zeros(256)
    for row in padded.reshape(rows, 256):
        part = part + row
    s = 128
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s >>= 1
    return float(dx) * part[0]


def section_terms(wx, wy, depth, qx, qy, counted=True):
    """(double)wx * Qx + (double)wy * Qy (two multiplies, one add) where the cell is counted and wet, +0.0 elsewhere."""
    hit = np.asarray(counted) & (depth > 1e-8)
    with np.errstate(all="ignore"):             # (cells that are not hit may hold anything)
        return np.where(hit, np.asarray(wx).astype(np.float64) * qx + np.asarray(wy).astype(np.float64) * qy, 0.0)


class ProbeRecorder:
    """The probe recorder in NumPy, in exactly the device kernel's operation order (csrc/hp_probes.hpp: record_probes; strided
    partial sums, then the halving tree): the reference the GPU tests compare against bit for bit, and the recorder of engines
    without the device path.  All arithmetic in fp64; only add, multiply and compare.

        ProbeRecorder(gauges, sections, dx)   gauges: (x, y) cell indices; sections: (cells, wx, wy) triples with cells as
                                              (x, y) pairs, or rasterise_section's objects
        record(state, bed, t)                 one sample: state[rows, cols, 4] = {Z, Zmax, Qx, Qy}, bed[rows, cols], t = the model time
        series()                              {"t": [n], "gauges": [n, G, 4] (z, depth, qx, qy), "sections": [n, S]} so far
    """

    def __init__(self, gauges=(), sections=(), dx=1.0):
        self.gauges = np.asarray(gauges, dtype=np.int64).reshape(-1, 2)
        self.sections = [Section(np.asarray(s[0], dtype=np.int64).reshape(-1, 2), np.asarray(s[1], np.int8).reshape(-1),
                                 np.asarray(s[2], np.int8).reshape(-1)) for s in sections]
        for s in self.sections:
            if not (len(s.cells) == len(s.wx) == len(s.wy) and len(s.cells) >= 2):
                raise ValueError("a section needs at least 2 cells and one weight pair per cell")
            if (np.abs(s.wx) > 1).any() or (np.abs(s.wy) > 1).any():
                raise ValueError("section weights are -1, 0 or 1")
        self.dx = float(dx)
        self.records = []

    @staticmethod
    def _cells(state, bed, cells):
        c = state[cells[:, 1], cells[:, 0]].astype(np.float64)
        zb = np.asarray(bed)[cells[:, 1], cells[:, 0]].astype(np.float64)
        z, zmax, qx, qy = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
        return z, z - zb, qx, qy, (zmax > -9999.0) & (zb <= 9999.0)           # counted as in domain_stats

    def record(self, state, bed, t):
        z, depth, qx, qy, counted = self._cells(state, bed, self.gauges)
        g = np.where(counted[:, None], np.stack([z, depth, qx, qy], axis=1), NODATA).reshape(-1, 4)
        q = []
        for s in self.sections:
            _, depth, qx, qy, counted = self._cells(state, bed, s.cells)
            q.append(fold_section_terms(section_terms(s.wx, s.wy, depth, qx, qy, counted), self.dx))
        self.records.append((float(t), g, np.array(q, np.float64)))

    def series(self):
        n, G, S = len(self.records), len(self.gauges), len(self.sections)
        return dict(t=np.array([r[0] for r in self.records], np.float64),
                    gauges=np.array([r[1] for r in self.records], np.float64).reshape(n, G, 4),
                    sections=np.array([r[2] for r in self.records], np.float64).reshape(n, S))


def write_probe_files(target_dir, series, gauge_names, section_names):
    """gauges.csv (time,name,fsl,depth,qx,qy) and sections.csv (time,name,discharge): one line per sample and probe, every
    number in its shortest exact decimal form (repr), so equal bits give equal bytes."""
    os.makedirs(target_dir, exist_ok=True)
    if gauge_names:
        with open(os.path.join(target_dir, "gauges.csv"), "w") as f:
            f.write("time,name,fsl,depth,qx,qy\n")
            for t, rec in zip(series["t"], series["gauges"]):
                for name, v in zip(gauge_names, rec):
                    f.write(",".join([repr(float(t)), name] + [repr(float(x)) for x in v]) + "\n")
    if section_names:
        with open(os.path.join(target_dir, "sections.csv"), "w") as f:
            f.write("time,name,discharge\n")
            for t, rec in zip(series["t"], series["sections"]):
                for name, v in zip(section_names, rec):
                    f.write(f"{float(t)!r},{name},{float(v)!r}\n")


# ------------------------------------------------------------------------------------------------ zones (areas)
ZONE_DEPTH_CAP = 1048576.0                      # csrc/hp_zones.hpp: 2^20 m, so that the scaled depth is an exact integer <= 2^52
ZONE_SCALE = 4294967296.0                       # 2^32: a depth is summed in units of 2^-32 m


def zone_ids(values, what="the zone raster"):
    """A raster of zone ids as uint16: every value an integer in 0..4096 (0 = in no zone), else ValueError."""
    a = np.asarray(values)
    if a.dtype.kind not in "iu":
        a = a.astype(np.float64)
        if not np.isfinite(a).all() or not np.array_equal(a, np.round(a)):
            raise ValueError(f"{what}: zone ids must be integers")
    if a.size and (a.min() < 0 or a.max() > ZONES_MAX):
        raise ValueError(f"{what}: zone ids must lie in 0..{ZONES_MAX}")
    return np.ascontiguousarray(a, dtype=np.uint16)


class ZoneRecorder:
    """The zone recorder in NumPy (csrc/hp_zones.hpp: record_zones): the reference the GPU tests compare against word for word, and
    the recorder of engines without the device path.  Floating-point operations in fp64, correctly rounded ones only; what is
    accumulated is unsigned 64-bit integers (np.add.at / np.maximum.at on uint64, never a float bincount), so the record does not
    depend on the order of the cells.

        ZoneRecorder(ids, zone_count, flood_depth, dx)   ids[rows, cols]: 0 = in no zone, 1..zone_count
        record(state, bed, t)                            one sample: state[rows, cols, 4] = {Z, Zmax, Qx, Qy}, bed[rows, cols]
        words()                                          uint64 [n, 1 + 7 zone_count]: hp_zones_read's layout
        series()                                         split_zone_records' dictionary
    """

    def __init__(self, ids, zone_count=None, flood_depth=0.1, dx=1.0):
        self.ids = zone_ids(ids)
        self.zone_count = int(zone_count) if zone_count is not None else max(1, int(self.ids.max()) if self.ids.size else 1)
        if not 1 <= self.zone_count <= ZONES_MAX:
            raise ValueError(f"zone_count outside 1..{ZONES_MAX}")
        if self.ids.size and int(self.ids.max()) > self.zone_count:
            raise ValueError("a zone id above zone_count")
        if not flood_depth >= 1e-8:
            raise ValueError("flood_depth must be at least 1e-8")
        self.flood_depth, self.dx = float(flood_depth), float(dx)
        self.records = []

    def record(self, state, bed, t):
        z, zmax, qx, qy = (np.asarray(state)[..., k].astype(np.float64) for k in range(4))
        zb = np.asarray(bed).astype(np.float64)
        if z.shape != self.ids.shape:
            raise ValueError("the state and the zone raster differ in shape")
        with np.errstate(all="ignore"):                                       # (cells that are not counted may hold anything)
            depth = z - zb
            counted = (zmax > -9999.0) & (zb <= 9999.0) & (self.ids != 0)     # domain_stats' rule, inside a zone
            d = np.where(depth > 0.0, depth, 0.0)
            d = np.where(d > ZONE_DEPTH_CAP, ZONE_DEPTH_CAP, d)
            q = np.rint(d * ZONE_SCALE).astype(np.uint64)                     # exact scaling, half to even
            wet = counted & (depth > 1e-8)
            flooded = counted & (depth > self.flood_depth)
            div = np.where(wet, depth, 1.0)                                   # (a dry cell's quotient is never formed)
            vx, vy = qx / div, qy / div
            sp = np.sqrt(vx * vx + vy * vy)
            fast = wet & (sp > 0.0)                                           # (a NaN or a zero contributes nothing)
        words = np.zeros((self.zone_count + 1, ZONE_WORDS), np.uint64)        # row 0: scratch, dropped below
        one = np.uint64(1)
        np.add.at(words[:, 0], self.ids[counted], one)
        np.add.at(words[:, 1], self.ids[wet], one)
        np.add.at(words[:, 2], self.ids[flooded], one)
        np.add.at(words[:, 3], self.ids[counted], q[counted] >> np.uint64(32))
        np.add.at(words[:, 4], self.ids[counted], q[counted] & np.uint64(0xffffffff))
        np.maximum.at(words[:, 5], self.ids[counted], np.ascontiguousarray(d[counted]).view(np.uint64))
        np.maximum.at(words[:, 6], self.ids[fast], np.ascontiguousarray(sp[fast]).view(np.uint64))
        rec = np.empty(1 + ZONE_WORDS * self.zone_count, np.uint64)
        rec[0] = np.array([float(t)], np.float64).view(np.uint64)[0]
        rec[1:] = words[1:].reshape(-1)
        self.records.append(rec)

    def words(self):
        return np.array(self.records, np.uint64).reshape(len(self.records), 1 + ZONE_WORDS * self.zone_count)

    def series(self):
        return split_zone_records(self.words(), self.zone_count, self.dx)


def combine_zones(parts):
    """The zone records of the whole grid from those of its parts (uint64 [n, 1 + 7 Z] each, hp_zones_read's layout; None entries
    are skipped), every cell counted in exactly one part: counts and depth limbs added, the two maxima taken.  Integer sums and
    maxima: equal to the single domain's record in every word, whatever the cut."""
    parts = [np.asarray(p, dtype=np.uint64) for p in parts if p is not None]
    if not parts:
        raise ValueError("no part")
    out = parts[0].copy()
    z = out[:, 1:].reshape(len(out), -1, ZONE_WORDS)
    for p in parts[1:]:
        if p.shape != out.shape:
            raise ValueError("the parts' zone records differ in shape")
        if not np.array_equal(p[:, 0], out[:, 0]):
            raise RuntimeError("the parts' zone samples were taken at different model times")
        pz = p[:, 1:].reshape(len(p), -1, ZONE_WORDS)
        z[:, :, :5] += pz[:, :, :5]
        z[:, :, 5:] = np.maximum(z[:, :, 5:], pz[:, :, 5:])
    return out


def write_zone_file(target_dir, series, dx, zone_names=None):
    """zones.csv (time,zone,cells,wet_area,flooded_area,volume,max_depth,max_speed): one line per sample and zone, areas = counts
    x dx^2, every number in its shortest exact decimal form (repr), so equal words give equal bytes."""
    os.makedirs(target_dir, exist_ok=True)
    area = float(dx) * float(dx)
    zones = series["cells"].shape[1]
    names = list(zone_names) if zone_names else [str(k + 1) for k in range(zones)]
    with open(os.path.join(target_dir, "zones.csv"), "w") as f:
        f.write("time,zone,cells,wet_area,flooded_area,volume,max_depth,max_speed\n")
        for n, t in enumerate(series["t"]):
            for k, name in enumerate(names):
                f.write(",".join([repr(float(t)), name, str(int(series["cells"][n, k])), repr(float(int(series["wet"][n, k]) * area)),
                                  repr(float(int(series["flooded"][n, k]) * area)), repr(float(series["volume"][n, k])),
                                  repr(float(series["max_depth"][n, k])), repr(float(series["max_speed"][n, k]))]) + "\n")


class BedShapes:
    """The moving bed on the host (hp_bed_shape_add / hp_bed_apply restated in NumPy, in exactly the kernel's operation order --
    csrc/hp_bed.hpp): shapes of cells with a target elevation each and one (time, fraction) series per shape.  `apply` acts in
    place on state[rows, cols, 4] and bed[rows, cols]; their dtype decides the single rounding.  All arithmetic is fp64 -- separate,
    correctly rounded multiplies, adds and divides -- so the arrays equal the device's bit for bit.  The GPU tests' reference, and
    what engines without the device path run (Model with the oracle's simulation objects)."""

    MAX_SHAPES, MAX_SERIES, MAX_CELLS, MAX_LEVEL = 64, 4096, 1048576, 9999.0

    def __init__(self, rows, cols):
        self.rows, self.cols = int(rows), int(cols)
        self.shapes = []                                # (flat cells, target, series, base or None)
        self.applies = 0

    def add(self, cells, target, series, bed=None):
        """`cells`: flat ids y * cols + x or (x, y) pairs.  `bed`: the bed the shape's base is captured from now (as the device does);
        without it the base is taken from the bed of the first apply."""
        c = np.asarray(cells)
        if c.ndim == 2 and c.shape[1] == 2:
            c = c[:, 1].astype(np.int64) * self.cols + c[:, 0].astype(np.int64)
        c = np.asarray(c, dtype=np.int64).reshape(-1)
        t = np.array(np.broadcast_to(np.asarray(target, dtype=np.float64), c.shape))
        s = np.array(series, dtype=np.float64).reshape(-1, 2)
        if not 1 <= len(s) <= self.MAX_SERIES:
            raise ValueError("series entries outside 1..4096")
        if not 1 <= c.size or sum(len(x[0]) for x in self.shapes) + c.size > self.MAX_CELLS:
            raise ValueError("cell count outside 1..1048576 over all shapes")
        if len(self.shapes) >= self.MAX_SHAPES:
            raise ValueError("more than 64 shapes")
        if not np.isfinite(t).all() or (np.abs(t) > self.MAX_LEVEL).any():
            raise ValueError("a target is not a finite elevation of at most 9999")
        if not np.isfinite(s[:, 0]).all() or not (np.diff(s[:, 0]) > 0).all():
            raise ValueError("times must be finite and strictly increasing")
        if not ((s[:, 1] >= 0.0) & (s[:, 1] <= 1.0)).all():
            raise ValueError("a fraction lies outside [0, 1]")
        if c.min() < 0 or c.max() >= self.rows * self.cols:
            raise ValueError("a cell lies outside the grid")
        everyone = np.concatenate([x[0] for x in self.shapes] + [c])
        uniq, counts = np.unique(everyone, return_counts=True)
        if (counts > 1).any():
            raise ValueError(f"cell {int(uniq[counts > 1][0])} is listed twice")
        base = None if bed is None else np.asarray(bed).reshape(-1)[c].astype(np.float64)
        self.shapes.append([c, t, s, base])

    @staticmethod
    def series_fraction(series, t):
        """bed_fraction of csrc/hp_bed.hpp: Python floats are IEEE doubles and nothing is fused."""
        s, t = np.asarray(series, dtype=np.float64).reshape(-1, 2), float(t)
        n = len(s)
        if not t > float(s[0, 0]):
            return float(s[0, 1])
        if t >= float(s[n - 1, 0]):
            return float(s[n - 1, 1])
        lo, hi = 0, n - 1
        while hi - lo > 1:
            mid = lo + (hi - lo) // 2
            if float(s[mid, 0]) <= t:
                lo = mid
            else:
                hi = mid
        t0, f0, t1, f1 = float(s[lo, 0]), float(s[lo, 1]), float(s[hi, 0]), float(s[hi, 1])
        df = f1 - f0
        part = (t - t0) / (t1 - t0)
        step = df * part
        return f0 + step

    @staticmethod
    def level(base, target, f):
        """bed_level of csrc/hp_bed.hpp on fp64 arrays: the new bed before it is rounded to the domain's precision."""
        base, target = np.asarray(base, dtype=np.float64), np.asarray(target, dtype=np.float64)
        if f <= 0.0:
            return base.copy()
        if f >= 1.0:
            return target.copy()
        rise = target - base
        part = np.float64(f) * rise
        return base + part

    def fraction(self, t):
        """One fraction per shape at time t."""
        return [self.series_fraction(s, t) for _, _, s, _ in self.shapes]

    def apply(self, state, bed, t):
        """One apply at time t, in place; returns the number of cells changed (skipped cells do not count)."""
        if state.shape != (self.rows, self.cols, 4) or bed.shape != (self.rows, self.cols) or state.dtype != bed.dtype or \
                not (state.flags.c_contiguous and bed.flags.c_contiguous):
            raise ValueError("state must be [rows, cols, 4] and bed [rows, cols], contiguous and of one dtype")
        real = bed.dtype.type
        st, zb = state.reshape(-1, 4), bed.reshape(-1)
        changed = 0
        for shape in self.shapes:
            c, target, series, base = shape
            if base is None:
                base = shape[3] = zb[c].astype(np.float64)
            f = self.series_fraction(series, t)
            b1_ = self.level(base, target, f).astype(real)
            b0_ = zb[c]
            b0, b1 = b0_.astype(np.float64), b1_.astype(np.float64)
            z0, zmax0 = st[c, 0].astype(np.float64), st[c, 1].astype(np.float64)
            with np.errstate(invalid="ignore"):
                move = (zmax0 > -9999.0) & (b0 <= 9999.0) & ~(b1_ == b0_)
                depth = z0 - b0
                z1 = b1 + depth
                zmax1 = np.where(zmax0 > z1, zmax0, z1)
            k = c[move]
            st[k, 0] = z1[move].astype(real)
            st[k, 1] = zmax1[move].astype(real)
            zb[k] = b1_[move]
            changed += int(move.sum())
        self.applies += 1
        return changed


class Links:
    """Link groups on the host (hp_boundary_add_links restated in NumPy, in exactly the operation order of csrc/hp_links.hpp:
    link_flow and link_record): weirs, orifices / culverts and pumps between two distant cells.  `apply` acts in place on
    state[rows, cols, 4], the iteration's source buffer, where the engine launches bdy_links; the arrays' dtype decides the single
    rounding of a stored level.  All arithmetic is fp64 -- separate, correctly rounded adds, multiplies, divides and square roots
    -- so state and records equal the device's bit for bit.  The GPU tests' reference; it also counts which branch each link took."""

    WEIR, ORIFICE, PUMP = 0, 1, 2
    MAX_LINKS = 65536
    G = 9.81
    BRANCHES = ("inert", "flap_shut", "weir_free", "weir_submerged", "weir_dry", "orifice_free", "orifice_capped", "orifice_dry",
                "pump_on", "pump_off", "avail_cap", "avail_none", "equalised")

    def __init__(self, rows, cols, dx, links, scheme_reach=1):
        from . import pack_links
        self.rows, self.cols, self.dx = int(rows), int(cols), float(dx)
        L = pack_links(links, self.cols)
        self.links = L
        n = len(L)
        if not 1 <= n <= self.MAX_LINKS:
            raise ValueError("link count outside 1..65536")
        if not np.isin(L["kind"], (0, 1, 2)).all():
            raise ValueError("unknown link kind")
        pump, weir, orifice = L["kind"] == 2, L["kind"] == 0, L["kind"] == 1
        if not (np.isfinite(L["level"]) & np.isfinite(L["size"])).all() or (L["size"] < 0).any():
            raise ValueError("level and size must be finite, size not negative")
        if not np.isfinite(L["coeff"][~pump]).all() or (L["coeff"][~pump] < 0).any():
            raise ValueError("coeff must be finite and not negative")
        with np.errstate(over="ignore"):
            if not np.isfinite((L["coeff"] * L["size"])[~pump]).all():
                raise ValueError("coeff * size must be finite")
        with np.errstate(invalid="ignore"):
            if not ((L["limit"][weir] >= 0) & (L["limit"][weir] < 1)).all() or not (L["limit"][orifice] >= 0).all():
                raise ValueError("a limit lies outside its range")
        ends = np.concatenate([L["cell_a"], L["cell_b"]]).astype(np.int64)
        if (L["cell_a"] == L["cell_b"]).any():
            raise ValueError("a link joins a cell to itself")
        if ends.max() >= self.rows * self.cols:
            raise ValueError("a link's cell lies outside the grid")
        y, x = ends // self.cols, ends % self.cols
        w = int(scheme_reach)
        if ((x < w) | (x + w >= self.cols) | (y < w) | (y + w >= self.rows)).any():
            raise ValueError("a link's cell lies on the grid's ring")
        uniq, counts = np.unique(ends, return_counts=True)
        if (counts > 1).any():
            raise ValueError(f"cell {int(uniq[counts > 1][0])} is an end of two links")
        self.a, self.b = L["cell_a"].astype(np.int64), L["cell_b"].astype(np.int64)
        self.q_last, self.volume, self.active = np.zeros(n), np.zeros(n), np.zeros(n, np.uint64)
        self.applies = 0
        self.branches = {k: np.zeros(n, np.int64) for k in self.BRANCHES}    # per link: iterations in which it took the branch

    def records(self):
        from . import LINK_RECORD_DTYPE
        out = np.zeros(len(self.links), LINK_RECORD_DTYPE)
        out["q_last"], out["volume"], out["active"] = self.q_last, self.volume, self.active
        return out

    def branch_totals(self):
        return {k: int(v.sum()) for k, v in self.branches.items()}

    def flow(self, za, zmax_a, bed_a, zb, zmax_b, bed_b, dt, dx, count=True):
        """link_flow on fp64 arrays, one element per link -> (za1, zb1, dz, s, inert): the levels before they are rounded."""
        L = self.links
        kind, level, size, coeff, limit = L["kind"], L["level"], L["size"], L["coeff"], L["limit"]
        dt, dx = np.float64(dt), np.float64(dx)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            inert = (dt <= 0.0) | ~((zmax_a > -9999.0) & (bed_a <= 9999.0)) | ~((zmax_b > -9999.0) & (bed_b <= 9999.0))
            a_up = np.where(kind == self.PUMP, True, za >= zb)
            zup, zdn, bed_up = np.where(a_up, za, zb), np.where(a_up, zb, za), np.where(a_up, bed_a, bed_b)
            s = np.where(a_up, 1.0, -1.0)
            shut = (L["one_way"] != 0) & ~a_up
            # weir
            hu = zup - level
            w_wet = hu > 0.0
            hu_ = np.where(w_wet, hu, 1.0)                                  # (lanes that take no root get a harmless operand)
            q_w = ((coeff * size) * hu_) * np.sqrt(hu_)
            hd = zdn - level
            sub = w_wet & (hd > limit * hu_)
            ratio = np.where(sub, (hu_ - hd) / (hu_ * (1.0 - limit)), 1.0)
            q_w = np.where(sub, q_w * np.sqrt(ratio), q_w)
            q_w = np.where(w_wet, q_w, 0.0)
            # orifice
            o_wet = zup > level
            dh = np.where(o_wet, zup - np.where(zdn > level, zdn, level), 0.0)
            free_q = (coeff * size) * np.sqrt((2.0 * self.G) * dh)
            capped = o_wet & (limit < free_q)
            q_o = np.where(o_wet, np.where(limit < free_q, limit, free_q), 0.0)
            # pump
            on = za > level
            q_p = np.where(on, size, 0.0)
            q = np.where(shut, 0.0, np.where(kind == self.WEIR, q_w, np.where(kind == self.ORIFICE, q_o, q_p)))
            dz = (q * dt) / (dx * dx)
            avail = zup - np.where(level > bed_up, level, bed_up)
            none = ~(avail > 0.0)
            cap = ~none & (avail < dz)
            dz = np.where(none, 0.0, np.where(cap, avail, dz))
            half = 0.5 * (zup - zdn)
            equal = (kind != self.PUMP) & (half < dz)
            dz = np.where(equal, half, dz)
            dz = np.where(inert, 0.0, dz)
            move = ~inert & (dz > 0.0)
            zup1, zdn1 = zup - dz, zdn + dz
            za1 = np.where(move, np.where(a_up, zup1, zdn1), za)
            zb1 = np.where(move, np.where(a_up, zdn1, zup1), zb)
        if count:
            live, B = ~inert, self.branches
            run = live & ~shut
            for name, mask in (("inert", inert), ("flap_shut", live & shut),
                               ("weir_free", run & (kind == 0) & w_wet & ~sub), ("weir_submerged", run & (kind == 0) & sub),
                               ("weir_dry", run & (kind == 0) & ~w_wet),
                               ("orifice_free", run & (kind == 1) & o_wet & ~capped), ("orifice_capped", run & (kind == 1) & capped),
                               ("orifice_dry", run & (kind == 1) & ~o_wet),
                               ("pump_on", run & (kind == 2) & on), ("pump_off", run & (kind == 2) & ~on),
                               ("avail_cap", live & cap & (q > 0.0)), ("avail_none", live & none & (q > 0.0)),
                               ("equalised", live & equal & (q > 0.0))):
                B[name] += mask
        return za1, zb1, dz, s, inert

    def apply(self, state, bed, dt):
        """One iteration's links, in place on `state` (the iteration's source buffer); `dt`: the timestep scalar of that iteration.
        Returns the number of links that moved water."""
        if state.shape != (self.rows, self.cols, 4) or bed.shape != (self.rows, self.cols) or not state.flags.c_contiguous:
            raise ValueError("state must be a contiguous [rows, cols, 4] and bed [rows, cols]")
        real = state.dtype.type
        st, zb = state.reshape(-1, 4), np.asarray(bed).reshape(-1)
        dt, dx = np.float64(real(dt)), np.float64(real(self.dx))
        a, b = self.a, self.b
        za1, zb1, dz, s, inert = self.flow(st[a, 0].astype(np.float64), st[a, 1].astype(np.float64), zb[a].astype(np.float64),
                                           st[b, 0].astype(np.float64), st[b, 1].astype(np.float64), zb[b].astype(np.float64), dt, dx)
        move = ~inert & (dz > 0.0)
        st[a[move], 0] = za1[move].astype(real)
        st[b[move], 0] = zb1[move].astype(real)
        with np.errstate(invalid="ignore", divide="ignore"):
            moved = dz * (dx * dx)
            self.q_last = np.where(inert, 0.0, s * (moved / dt))
            self.volume = np.where(inert, self.volume, self.volume + s * moved)
        self.active = self.active + move.astype(np.uint64)
        self.applies += 1
        return int(move.sum())


class Open:
    """The open boundary on the host (hp_boundary_add_open restated in NumPy, in exactly the operation order of csrc/hp_open.hpp:
    open_impose and open_record): segments of the edge ring whose cells take the depth and the outward momentum of their inward
    neighbours and record the discharge that leaves through their faces.  `apply` acts in place on state[rows, cols, 4], the
    iteration's source buffer, where the engine launches bdy_open; the arrays' dtype decides the single rounding of a stored value.
    The face mass flux comes from `functions` -- an object with the oracle's `reconstruct` and `hllc` in the state's precision
    (oracle.OracleFunctions), called in godunov_cell's argument order as frontend.Tracer.face_fluxes calls them; everything else is
    fp64: separate, correctly rounded adds, subtracts and multiplies, so state and records equal the device's bit for bit.  The GPU
    tests' reference; it also counts which branch each cell took.  `segments`: see pack_open_segments (GLOBAL indices); a strip
    (row_offset, global_rows) keeps the ring cells whose row lies in its `rows` local rows."""

    SOUTH, NORTH, WEST, EAST = 0, 1, 2, 3
    MAX_SEGMENTS = 64
    DIRECTION = {0: 2, 1: 0, 2: 3, 3: 1}                   # the edge's face of the inward neighbour, as Tracer.DIR_*
    # per cell and iteration: inert, or any of dry (d == 0), level_capped (step 3's cap), inward_zeroed (an inward Qn_i was not taken),
    # and one of outflow (out > 0) / inflow (out < 0) / neither
    BRANCHES = ("inert", "dry", "level_capped", "inward_zeroed", "outflow", "inflow")

    def __init__(self, rows, cols, dx, functions, segments, row_offset=0, global_rows=None, dry_threshold=1e-10):
        from . import pack_open_segments
        self.rows, self.cols, self.row_offset = int(rows), int(cols), int(row_offset)
        self.global_rows = self.rows if global_rows is None else int(global_rows)
        self.fn = functions
        self.real = np.dtype(functions.real).type
        self.dx = np.float64(self.real(dx))                                    # dx as the kernels hold it
        self.vs = self.real(dry_threshold)
        if segments is None:
            raise ValueError("segments == NULL")
        S = pack_open_segments(segments, self.cols, self.global_rows)
        if len(S) < 1:
            raise ValueError("count == 0")
        if len(S) > self.MAX_SEGMENTS:
            raise ValueError("more than 64 segments on the domain")
        edge, seg, at = [], [], []
        for k, s in enumerate(S):
            if int(s["edge"]) not in (0, 1, 2, 3):
                raise ValueError(f"segment {k}: unknown edge")
            if int(s["reserved"]) != 0:
                raise ValueError(f"segment {k}: reserved must be 0")
            if s["first"] > s["last"]:
                raise ValueError(f"segment {k}: first > last")
            n = self.cols if int(s["edge"]) in (self.SOUTH, self.NORTH) else self.global_rows
            if s["first"] < 1 or s["last"] > n - 2:
                raise ValueError(f"segment {k}: index {int(s['first']) if s['first'] < 1 else n - 1} lies outside 1..{n - 2}")
            idx = np.arange(int(s["first"]), int(s["last"]) + 1)
            at.append(idx); edge.append(np.full(len(idx), int(s["edge"]))); seg.append(np.full(len(idx), k))
        self.segments = S
        self.edge, self.segment_of, at = np.concatenate(edge), np.concatenate(seg), np.concatenate(at)
        e, last_row, last_col = self.edge, self.global_rows - 1, self.cols - 1
        # the ring cell and its inward neighbour as (column, GLOBAL row)
        self.rx = np.where(e == self.WEST, 0, np.where(e == self.EAST, last_col, at))
        self.ry = np.where(e == self.SOUTH, 0, np.where(e == self.NORTH, last_row, at))
        self.ix = np.where(e == self.WEST, 1, np.where(e == self.EAST, last_col - 1, at))
        self.iy = np.where(e == self.SOUTH, 1, np.where(e == self.NORTH, last_row - 1, at))
        self.cells = self.ry.astype(np.int64) * self.cols + self.rx            # GLOBAL flat ids of the listed ring cells, in the records' order
        uniq, first_at, counts = np.unique(self.cells, return_index=True, return_counts=True)
        if (counts > 1).any():
            twice = int(uniq[counts > 1][0])
            later = int(self.segment_of[np.flatnonzero(self.cells == twice)[1]])
            raise ValueError(f"segment {later}: cell {twice} is listed twice")
        lo, hi = self.row_offset, self.row_offset + self.rows
        self.kept = (self.ry >= lo) & (self.ry < hi) & (self.iy >= lo) & (self.iy < hi)      # the strip's selection
        n = len(self.cells)
        self.q_last, self.volume, self.active = np.zeros(n), np.zeros(n), np.zeros(n, np.uint64)
        self.applies = 0
        self.branches = {k: np.zeros(n, np.int64) for k in self.BRANCHES}    # per cell: iterations in which it took the branch

    def records(self):
        from . import OPEN_RECORD_DTYPE
        out = np.zeros(len(self.cells), OPEN_RECORD_DTYPE)
        out["q_last"], out["volume"], out["active"] = self.q_last, self.volume, self.active
        return out

    def branch_totals(self):
        return {k: int(v.sum()) for k, v in self.branches.items()}

    def segment_totals(self):
        """Per segment (discharge, volume): math.fsum over its cells' records -- exactly rounded, so independent of any order."""
        import math
        return [(math.fsum(self.q_last[self.segment_of == k]), math.fsum(self.volume[self.segment_of == k])) for k in range(len(self.segments))]

    @staticmethod
    def impose(edge, zmax_r, bed_r, z_i, zmax_i, qn_i, qs_i, bed_i, dt):
        """open_impose on fp64 arrays, one element per cell -> (inert, lvl, qn, qs, dry, capped, zeroed): the level before it is rounded."""
        a = lambda v: np.asarray(v, dtype=np.float64)
        zmax_r, bed_r, z_i, zmax_i, qn_i, qs_i, bed_i = (a(v) for v in (zmax_r, bed_r, z_i, zmax_i, qn_i, qs_i, bed_i))
        edge, dt = np.asarray(edge), np.asarray(dt, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            inert = (dt <= 0.0) | ~((zmax_r > -9999.0) & (bed_r <= 9999.0)) | ~((zmax_i > -9999.0) & (bed_i <= 9999.0))
            d = z_i - bed_i
            d = np.where(d > 0.0, d, 0.0)
            lvl = bed_r + d
            capped = lvl > z_i
            lvl = np.where(capped, np.where(z_i > bed_r, z_i, bed_r), lvl)
            dry = d == 0.0
            positive = (edge == Open.EAST) | (edge == Open.NORTH)
            outward = np.where(positive, qn_i > 0.0, qn_i < 0.0)
            qn = np.where(~dry & outward, qn_i, 0.0)
            qs = np.where(~dry, qs_i, 0.0)
            zeroed = ~dry & ~outward & (qn_i != 0.0)
        live = ~inert
        return inert, lvl, qn, qs, live & dry, live & capped, live & zeroed

    @staticmethod
    def record(q_last, volume, active, inert, edge, F, dt, dx):
        """open_record on fp64 arrays -> (q_last, volume, active, out)."""
        F, dt, dx = (np.asarray(v, dtype=np.float64) for v in (F, dt, dx))
        inert = np.asarray(inert, dtype=bool)
        positive = (np.asarray(edge) == Open.EAST) | (np.asarray(edge) == Open.NORTH)
        with np.errstate(invalid="ignore", over="ignore"):
            out = np.where(positive, F, -F)
            q1 = np.where(inert, 0.0, out * dx)
            v1 = np.where(inert, volume, volume + (out * dt) * dx)
            a1 = np.asarray(active, dtype=np.uint64) + (~inert & (out > 0.0)).astype(np.uint64)
        return q1, v1, a1, out

    def face_flux(self, state, bed, k):
        """F of listed cell k (local rows): the face between the inward neighbour and the ring cell as godunov_cell forms it for the
        neighbour (Tracer.face_fluxes' statement for that face)."""
        f, direction = self.fn, self.DIRECTION[int(self.edge[k])]
        ry, iy, rx, ix = int(self.ry[k]) - self.row_offset, int(self.iy[k]) - self.row_offset, int(self.rx[k]), int(self.ix[k])
        if int(self.edge[k]) in (self.EAST, self.NORTH):
            L, R, _ = f.reconstruct(direction, state[iy, ix], bed[iy, ix], state[ry, rx], bed[ry, rx])
        else:
            L, R, _ = f.reconstruct(direction, state[ry, rx], bed[ry, rx], state[iy, ix], bed[iy, ix])
        return f.hllc(direction, L, R)[0]

    def apply(self, state, bed, dt):
        """One iteration's open boundary, in place on `state` (the iteration's source buffer); `dt`: the timestep scalar of that
        iteration.  Returns the number of cells through which water left."""
        if state.shape != (self.rows, self.cols, 4) or bed.shape != (self.rows, self.cols) or state.dtype != bed.dtype:
            raise ValueError("state must be [rows, cols, 4] and bed [rows, cols], of one dtype")
        if state.dtype.type is not self.real:
            raise ValueError("the face-flux functions and the state differ in precision")
        real = self.real
        dt64 = np.float64(real(dt))
        kept = np.flatnonzero(self.kept)
        e = self.edge[kept]
        ry, iy, rx, ix = self.ry[kept] - self.row_offset, self.iy[kept] - self.row_offset, self.rx[kept], self.ix[kept]
        along_x = (e == self.WEST) | (e == self.EAST)
        inner = state[iy, ix].astype(np.float64)
        qn_i, qs_i = np.where(along_x, inner[:, 2], inner[:, 3]), np.where(along_x, inner[:, 3], inner[:, 2])
        inert, lvl, qn, qs, dry, capped, zeroed = self.impose(e, state[ry, rx, 1].astype(np.float64), bed[ry, rx].astype(np.float64), inner[:, 0], inner[:, 1],
                                                              qn_i, qs_i, bed[iy, ix].astype(np.float64), dt64)
        live = ~inert
        z_new = lvl.astype(real)
        ring = state[ry, rx]
        ring[:, 0] = np.where(live, z_new, ring[:, 0])
        ring[:, 1] = np.where(live & ~(ring[:, 1] > z_new), z_new, ring[:, 1])
        ring[:, 2] = np.where(live, np.where(along_x, qn, qs).astype(real), ring[:, 2])
        ring[:, 3] = np.where(live, np.where(along_x, qs, qn).astype(real), ring[:, 3])
        state[ry, rx] = ring
        F = np.zeros(len(kept))
        for j in np.flatnonzero(live):
            F[j] = np.float64(self.face_flux(state, bed, int(kept[j])))
        q1, v1, a1, out = self.record(self.q_last[kept], self.volume[kept], self.active[kept], inert, e, F, dt64, self.dx)
        self.q_last[kept], self.volume[kept], self.active[kept] = q1, v1, a1
        for name, mask in (("inert", inert), ("dry", dry), ("level_capped", capped), ("inward_zeroed", zeroed),
                           ("outflow", live & (out > 0.0)), ("inflow", live & (out < 0.0))):
            self.branches[name][kept] += mask
        self.applies += 1
        return int((live & (out > 0.0)).sum())


class Infiltration:
    """The infiltration on the host (hp_boundary_add_infiltration restated in NumPy, in exactly the operation order of
    csrc/hp_soil.hpp: soil_step): Green-Ampt by soil class.  `apply` acts in place on state[rows, cols, 4], the iteration's source
    buffer, where the engine launches bdy_infiltration; the arrays' dtype decides the single rounding of a stored level.  All
    arithmetic is fp64 -- separate, correctly rounded adds, multiplies and square roots -- so the state and F equal the device's bit
    for bit.  The GPU tests' reference; it also counts which branch each cell took."""

    BRANCHES = ("ring", "impervious", "not_counted", "dry", "potential", "depth_limited", "capacity_cap", "capacity_full")

    def __init__(self, rows, cols, classes, soil, initial=None, row_offset=0, global_rows=None):
        """`row_offset`, `global_rows`: where the rows of a strip's local array lie in the whole grid (default: the whole grid)."""
        from . import pack_soil_classes, soil_ids
        self.rows, self.cols = int(rows), int(cols)
        # the grid's edge ring (csrc/hp_soil.hpp: soil_on_ring): the outermost cells of the GLOBAL grid are left alone
        gy = np.arange(self.rows) + int(row_offset)
        x = np.arange(self.cols)
        top = (self.rows if global_rows is None else int(global_rows)) - 1
        self.ring = ((gy <= 0) | (gy >= top))[:, None] | ((x <= 0) | (x >= self.cols - 1))[None, :]
        self.classes = c = pack_soil_classes(classes)
        n = len(c)
        if not 1 <= n <= 255:
            raise ValueError("class_count outside 1..255")
        if not (np.isfinite(c["ks"]) & np.isfinite(c["suction"])).all() or (c["ks"] < 0).any() or (c["suction"] < 0).any():
            raise ValueError("ks and suction must be finite and not negative")
        with np.errstate(invalid="ignore", over="ignore"):
            if not ((c["deficit"] >= 0) & (c["deficit"] <= 1)).all():
                raise ValueError("the moisture deficit lies in [0, 1]")
            if not (c["capacity"] >= 0).all():
                raise ValueError("the capacity is >= 0 (+inf for none)")
            if not np.isfinite(c["ks"] * 1e6).all() or not np.isfinite(c["suction"] * c["deficit"]).all():
                raise ValueError("ks * 1e6 and suction * deficit must be finite")
        self.soil = soil_ids(soil)
        if self.soil.shape != (self.rows, self.cols):
            raise ValueError(f"the soil raster must be [{self.rows}, {self.cols}]")
        if int(self.soil.max(initial=0)) > n:
            bad = int(np.flatnonzero(self.soil.reshape(-1) > n)[0])
            raise ValueError(f"cell {bad} has a class id above class_count")
        if initial is None:
            self.F = np.zeros((self.rows, self.cols))
        else:
            self.F = np.array(initial, dtype=np.float64)
            if self.F.shape != (self.rows, self.cols):
                raise ValueError(f"the initial infiltration must be [{self.rows}, {self.cols}]")
            if not np.isfinite(self.F).all() or (self.F < 0).any():
                bad = int(np.flatnonzero(~(np.isfinite(self.F) & (self.F >= 0)).reshape(-1))[0])
                raise ValueError(f"cell {bad}: initial must be finite and >= 0")
        # the class table indexed by the id itself (entry 0 is never used), S formed once
        self.ks, self.S, self.capacity = (np.zeros(n + 1) for _ in range(3))
        self.ks[1:], self.S[1:], self.capacity[1:] = c["ks"], c["suction"] * c["deficit"], c["capacity"]
        self.applies = 0
        self.branches = {k: np.zeros((self.rows, self.cols), np.int64) for k in self.BRANCHES}   # per cell: iterations in which it took the branch

    def branch_totals(self):
        return {k: int(v.sum()) for k, v in self.branches.items()}

    @staticmethod
    def step(ks, S, capacity, F, z, zmax, bed, dt):
        """soil_step on fp64 arrays, one element per cell of a class other than 0 -> (dF, z1, masks): the level before it is rounded,
        and which branch each element took."""
        dt = np.float64(dt)
        with np.errstate(invalid="ignore", over="ignore"):
            counted = (zmax > -9999.0) & (bed <= 9999.0)
            depth = z - bed
            wet = depth > 0.0
            kd = ks * dt
            b = kd - 2.0 * F
            disc = b * b + (8.0 * kd) * (S + F)
            root = np.sqrt(np.where(disc >= 0.0, disc, 0.0))                 # (disc is a sum of two non-negative terms, or a NaN)
            root = np.where(disc >= 0.0, root, np.nan)
            pot = 0.5 * (b + root)
            pot = np.where(pot > 0.0, pot, 0.0)
            room = capacity - F
            full = ~(room > 0.0)
            capped = ~full & (room < pot)
            pot = np.where(full, 0.0, np.where(capped, room, pot))
            limited = depth < pot
            dF = np.where(limited, depth, pot)
            live = counted & wet & (dt > 0.0)
            dF = np.where(live & (dF > 0.0), dF, 0.0)
            z1 = np.where(dF > 0.0, z - dF, z)
        masks = dict(not_counted=~counted, dry=counted & ~wet, capacity_full=live & full, depth_limited=live & ~full & limited,
                     capacity_cap=live & capped & ~limited, potential=live & ~full & ~capped & ~limited)
        return dF, z1, masks

    def apply(self, state, bed, dt):
        """One iteration's infiltration, in place on `state` (the iteration's source buffer) and on F; `dt`: the timestep scalar of
        that iteration.  Returns the number of cells changed."""
        if state.shape != (self.rows, self.cols, 4) or bed.shape != (self.rows, self.cols) or not state.flags.c_contiguous:
            raise ValueError("state must be a contiguous [rows, cols, 4] and bed [rows, cols]")
        real = state.dtype.type
        dt = np.float64(real(dt))
        self.applies += 1
        if not dt > 0.0:
            return 0
        st, zb, F, ids = state.reshape(-1, 4), np.asarray(bed).reshape(-1), self.F.reshape(-1), self.soil.reshape(-1)
        at = np.flatnonzero((ids != 0) & ~self.ring.reshape(-1))
        k = ids[at]
        dF, z1, masks = self.step(self.ks[k], self.S[k], self.capacity[k], F[at], st[at, 0].astype(np.float64), st[at, 1].astype(np.float64),
                                  zb[at].astype(np.float64), dt)
        move = dF > 0.0
        st[at[move], 0] = z1[move].astype(real)
        F[at[move]] = F[at[move]] + dF[move]
        self.branches["ring"] += self.ring
        self.branches["impervious"] += (self.soil == 0) & ~self.ring
        for name, mask in masks.items():
            self.branches[name].reshape(-1)[at] += mask
        return int(move.sum())


def _icbrt(n):
    """floor(n ** (1/3)) of a non-negative Python integer: Newton's iteration from above."""
    if n < 2:
        return n
    r = 1 << -(-n.bit_length() // 3)                                           # 2^ceil(bits / 3) >= the root
    while True:
        nxt = (2 * r + n // (r * r)) // 3
        if nxt >= r:
            return r
        r = nxt


def cbrt_exact(x):
    """The correctly rounded (to nearest) cube root of a positive, finite double, by integer arithmetic alone: the significand is scaled
    to an integer of more than 3 * 55 bits whose exponent is a multiple of three, its integer cube root taken, and the root rounded to
    53 bits.  A cube root of a double is never halfway between two doubles unless it is exact, so the remainder decides.  Independent of
    csrc/hp_crmath.h: what tests hold hp_cr_cbrt against, and the cube root of Tracer's bed shear stress."""
    x = float(x)
    if not (x > 0.0) or x == float("inf"):
        raise ValueError("cbrt_exact takes a positive, finite double")
    m, e = math.frexp(x)
    m, e = int(m * (1 << 53)), e - 53                                          # x = m * 2^e exactly, 2^52 <= m < 2^53
    k = 120 + (e - 120) % 3                                                    # m << k has 173 bits or more; e - k is a multiple of 3
    n = m << k
    r = _icbrt(n)
    exact = r * r * r == n
    drop = r.bit_length() - 53                                                 # >= 4: the root has 57 bits or more
    q, rem, half = r >> drop, r & ((1 << drop) - 1), 1 << (drop - 1)
    if rem > half or (rem == half and (not exact or q & 1)):               # (not exact: the true root lies above r)
        q += 1
    return math.ldexp(q, drop + (e - k) // 3)


def cbrt_exact_array(x):
    """cbrt_exact over an array of positive, finite doubles (each distinct value once)."""
    x = np.asarray(x, dtype=np.float64)
    values, where = np.unique(x.reshape(-1), return_inverse=True)
    roots = np.array([cbrt_exact(v) for v in values], dtype=np.float64)
    return roots[where].reshape(x.shape)


class Tracer:
    """The passive tracer on the host (hp_tracer_enable restated in NumPy, in exactly the operation order of csrc/hp_tracer.hpp):
    the solute mass per unit area M, fp64 whatever the state's precision.  `apply` is one iteration's tracer on the iteration's
    source buffer, where the engine launches tracer_sources and tracer_step: behind every boundary, in front of the flux step.
    The face mass fluxes come from `functions` -- an object with the oracle's `reconstruct(direction, sL, bL, sR, bR)` and
    `hllc(direction, L, R)` in the state's precision (oracle.OracleFunctions) -- called in godunov_cell's argument order; everything
    behind them is fp64: separate, correctly rounded adds, multiplies and divides, so M equals the device's bit for bit.  The GPU
    tests' reference; it also counts which branch each cell took."""

    MAX_SOURCES, MAX_SERIES, MAX_CELLS, DEPTH_MIN = 64, 4096, 1048576, 1e-10
    DIR_N, DIR_E, DIR_S, DIR_W = 0, 1, 2, 3
    # per cell and iteration: one of the copy cases or "moved"; for a moved cell, per face, which side gave its concentration
    # (_pos: the flux is > 0, _neg: it is not), and whether a cell too shallow to have a concentration was among the five
    BRANCHES = ("ring", "dt_zero", "disabled", "dry5", "moved", "e_pos", "e_neg", "w_pos", "w_neg", "n_pos", "n_neg", "s_pos", "s_neg",
                "no_concentration", "source")
    MAX_SPECIES = 8
    RHO_G = 9810.0                                      # rho g of the Manning bed shear stress, N/m3

    @staticmethod
    def exchange_params(exchange):
        """The four parameters of step 7 (hp_tracer_exchange_desc_t) as fp64, checked in the header's order."""
        unknown = set(exchange) - {"settling", "tau_deposit", "tau_erode", "erodibility"}
        if unknown:
            raise ValueError(f"exchange has no parameter {sorted(unknown)[0]!r}")
        ws, tcd = np.float64(exchange.get("settling", 0.0)), np.float64(exchange.get("tau_deposit", np.inf))
        tce, E = np.float64(exchange.get("tau_erode", np.inf)), np.float64(exchange.get("erodibility", 0.0))
        if not np.isfinite(ws) or ws < 0:
            raise ValueError("settling must be finite and >= 0")
        if not tcd > 0:
            raise ValueError("tau_deposit must be > 0 (+inf allowed)")
        if np.isnan(tce) or tce < tcd:
            raise ValueError("tau_erode must be >= tau_deposit (+inf allowed)")
        if not np.isfinite(E) or E < 0:
            raise ValueError("erodibility must be finite and >= 0")
        return dict(settling=ws, tau_deposit=tcd, tau_erode=tce, erodibility=E)

    def __init__(self, rows, cols, dx, functions, initial=None, dry_threshold=1e-10, decay=0.0, exchange=None, deposit=None, manning=0.0):
        self.decay = np.float64(decay)                                         # lambda of step 6 (a tracer set's species), 1 / s
        if not np.isfinite(self.decay) or self.decay < 0:
            raise ValueError("the decay rate must be finite and >= 0")
        self.exchange = None if exchange is None else self.exchange_params(exchange)   # step 7 (hp_tracer_set_exchange), or None
        self.rows, self.cols = int(rows), int(cols)
        self.fn = functions
        self.real = np.dtype(functions.real).type
        self.dx = np.float64(self.real(dx))                                    # dx as the kernels hold it
        self.vs = self.real(dry_threshold)
        if initial is None:
            self.M = np.zeros((self.rows, self.cols))
        else:
            self.M = np.array(initial, dtype=np.float64)
            if self.M.shape != (self.rows, self.cols):
                raise ValueError(f"the initial tracer must be [{self.rows}, {self.cols}]")
            if not np.isfinite(self.M).all() or (self.M < 0).any():
                bad = int(np.flatnonzero(~(np.isfinite(self.M) & (self.M >= 0)).reshape(-1))[0])
                raise ValueError(f"cell {bad}: initial must be finite and >= 0")
        # the deposit D of step 7 and the Manning values the flux kernel uses (a scalar or [rows, cols]), in the state's precision
        if deposit is None:
            self.D = np.zeros((self.rows, self.cols))
        else:
            self.D = np.array(deposit, dtype=np.float64)
            if self.D.shape != (self.rows, self.cols):
                raise ValueError(f"the initial deposit must be [{self.rows}, {self.cols}]")
            if not (np.isfinite(self.D) & (self.D >= 0)).all():
                bad = int(np.flatnonzero(~(np.isfinite(self.D) & (self.D >= 0)).reshape(-1))[0])
                raise ValueError(f"cell {bad}: deposit_initial must be finite and >= 0")
        self.manning = np.broadcast_to(np.asarray(manning, dtype=self.real), (self.rows, self.cols)).astype(np.float64)
        self.sources = []                               # (flat cells, series)
        self.iterations = 0
        self.branches = {k: np.zeros((self.rows, self.cols), np.int64) for k in self.BRANCHES + ("decayed", "deposited", "eroded")}

    def branch_totals(self):
        return {k: int(v.sum()) for k, v in self.branches.items()}

    def add_source(self, cells, series):
        """`cells`: flat ids y * cols + x or (x, y) pairs; `series`: [(time, mass rate)]."""
        c = np.asarray(cells)
        if c.ndim == 2 and c.shape[1] == 2:
            c = c[:, 1].astype(np.int64) * self.cols + c[:, 0].astype(np.int64)
        c = np.asarray(c, dtype=np.int64).reshape(-1)
        s = np.array(series, dtype=np.float64).reshape(-1, 2)
        if not 1 <= len(s) <= self.MAX_SERIES:
            raise ValueError("entries outside 1..4096")
        if not 1 <= c.size <= self.MAX_CELLS:
            raise ValueError("count outside 1..1048576")
        if not np.isfinite(s[:, 0]).all() or not (np.diff(s[:, 0]) > 0).all():
            raise ValueError("times must be finite and strictly increasing")
        if not np.isfinite(s[:, 1]).all():
            raise ValueError("the mass rate must be finite")
        if c.min() < 0 or c.max() >= self.rows * self.cols:
            raise ValueError("a cell lies outside the grid")
        y, x = c // self.cols, c % self.cols
        if ((x == 0) | (y == 0) | (x == self.cols - 1) | (y == self.rows - 1)).any():
            raise ValueError("a cell lies on the grid's edge ring")
        if len(self.sources) >= self.MAX_SOURCES:
            raise ValueError("more than 64 sources")
        everyone = np.concatenate([x[0] for x in self.sources] + [c])
        if everyone.size > self.MAX_CELLS:
            raise ValueError("more than 1048576 cells over all sources")
        uniq, counts = np.unique(everyone, return_counts=True)
        if (counts > 1).any():
            raise ValueError(f"cell {int(uniq[counts > 1][0])} is listed twice")
        self.sources.append((c, s))

    @staticmethod
    def source_step(M, rate, dt, dx):
        """tracer_source_add on fp64 arrays."""
        mass = np.float64(rate) * np.float64(dt)
        area = np.float64(dx) * np.float64(dx)
        add = mass / area
        return np.asarray(M, dtype=np.float64) + add

    @staticmethod
    def decay_step(M, lam, dt):
        """tracer_decay on fp64 arrays: step 6."""
        M, lam, dt = np.asarray(M, dtype=np.float64), np.float64(lam), np.float64(dt)
        if not (lam > 0.0 and dt > 0.0):
            return M
        with np.errstate(over="ignore", invalid="ignore"):
            growth = lam * dt
            denom = np.float64(1.0) + growth
            return M / denom

    def _decay(self, dt64):
        """Step 6 on the M the step left, at every cell of the array."""
        if self.decay > 0.0 and dt64 > 0.0:
            self.M = self.decay_step(self.M, self.decay, dt64)
            self.branches["decayed"] += 1

    @staticmethod
    def shear(h, qx, qy, n):
        """tracer_shear on fp64 arrays: the Manning bed shear stress of cells deeper than DEPTH_MIN (NaN elsewhere)."""
        h, qx, qy, n = (np.asarray(v, dtype=np.float64) for v in (h, qx, qy, n))
        deep = h > Tracer.DEPTH_MIN
        hh = np.where(deep, h, 1.0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            vx = qx / hh
            vy = qy / hh
            sp2 = vx * vx + vy * vy
            nn = n * n
            tau = ((np.float64(Tracer.RHO_G) * nn) * sp2) / cbrt_exact_array(hh)
        return np.where(deep, tau, np.nan)

    @staticmethod
    def exchange_step(M, D, h, qx, qy, n, dt, q, tau=None):
        """tracer_exchange on fp64 arrays: step 7 -> (M, D, deposited mask, eroded mask).  `q`: exchange_params' dict; `tau`: shear(h, qx,
        qy, n) if the caller has it already."""
        M, D, h = (np.asarray(v, dtype=np.float64) for v in (M, D, h))
        dt = np.float64(dt)
        ws, tcd, tce, E = q["settling"], q["tau_deposit"], q["tau_erode"], q["erodibility"]
        deep = h > Tracer.DEPTH_MIN
        tau = Tracer.shear(h, qx, qy, n) if tau is None else np.asarray(tau, dtype=np.float64)
        hh = np.where(deep, h, 1.0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            dep_at = deep & bool(ws > 0.0) & (M > 0.0) & (tau < tcd)
            pd = np.float64(1.0) if np.isinf(tcd) else np.float64(1.0) - tau / tcd
            k = (ws * pd) * dt
            r = k / hh
            M3 = M / (np.float64(1.0) + r)
            dep = M - M3
            ero_at = deep & ~dep_at & bool(E > 0.0) & (D > 0.0) & (tau > tce)
            ex = tau / tce - np.float64(1.0)
            ero = (E * ex) * dt
            ero = np.where(ero > D, D, ero)
            M_out = np.where(dep_at, M3, np.where(ero_at, M + ero, M))
            D_out = np.where(dep_at, D + dep, np.where(ero_at, D - ero, D))
        return M_out, D_out, dep_at, ero_at

    def _exchange(self, state, bed, ys, xs, dt64, shared):
        """Step 7 behind the decay, at the moved cells (ys, xs)."""
        q = self.exchange
        if q is None or not (q["settling"] > 0.0 or q["erodibility"] > 0.0):
            return
        if shared is None or "tau" not in shared:                             # the water's part: formed once for all species, as on the device
            h = state[ys, xs, 0].astype(np.float64) - bed[ys, xs].astype(np.float64)
            tau = self.shear(h, state[ys, xs, 2], state[ys, xs, 3], self.manning[ys, xs])
            if shared is not None:
                shared["h"], shared["tau"] = h, tau
        else:
            h, tau = shared["h"], shared["tau"]
        M, D, dep_at, ero_at = self.exchange_step(self.M[ys, xs], self.D[ys, xs], h, None, None, None, dt64, q, tau=tau)
        self.M = self.M.copy()
        self.D = self.D.copy()
        self.M[ys, xs], self.D[ys, xs] = M, D
        self.branches["deposited"][ys, xs] += dep_at
        self.branches["eroded"][ys, xs] += ero_at

    @staticmethod
    def concentration(M, h):
        """tracer_conc on fp64 arrays."""
        M, h = np.asarray(M, dtype=np.float64), np.asarray(h, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            return np.where(h > Tracer.DEPTH_MIN, M / np.where(h > Tracer.DEPTH_MIN, h, 1.0), 0.0)

    @staticmethod
    def update(M, cC, cN, cS, cE, cW, FN, FS, FE, FW, dt, dx):
        """tracer_update on fp64 arrays -> (M', masks): which side each face took."""
        a = lambda v: np.asarray(v, dtype=np.float64)
        M, cC, cN, cS, cE, cW, FN, FS, FE, FW = (a(v) for v in (M, cC, cN, cS, cE, cW, FN, FS, FE, FW))
        dt, dx = np.float64(dt), np.float64(dx)
        with np.errstate(invalid="ignore", over="ignore"):
            e, w, n, s = FE > 0.0, FW > 0.0, FN > 0.0, FS > 0.0
            GE = np.where(e, FE * cC, FE * cE)
            GW = np.where(w, FW * cW, FW * cC)
            GN = np.where(n, FN * cC, FN * cN)
            GS = np.where(s, FS * cS, FS * cC)
            ex = GE - GW
            ey = GN - GS
            total = ex + ey
            div = total / dx
            step = dt * div
            out = M - step
        return out, dict(e_pos=e, e_neg=~e, w_pos=w, w_neg=~w, n_pos=n, n_neg=~n, s_pos=s, s_neg=~s)

    def face_fluxes(self, state, bed, x, y):
        """FN, FS, FE, FW of cell (x, y) as godunov_cell forms them (oracle/swe_oracle.c:472-486), in the state's precision."""
        f = self.fn
        c, bC = state[y, x], bed[y, x]
        L, R, _ = f.reconstruct(self.DIR_N, c, bC, state[y + 1, x], bed[y + 1, x])
        FN = f.hllc(self.DIR_N, L, R)[0]
        L, R, _ = f.reconstruct(self.DIR_S, state[y - 1, x], bed[y - 1, x], c, bC)
        FS = f.hllc(self.DIR_S, L, R)[0]
        L, R, _ = f.reconstruct(self.DIR_E, c, bC, state[y, x + 1], bed[y, x + 1])
        FE = f.hllc(self.DIR_E, L, R)[0]
        L, R, _ = f.reconstruct(self.DIR_W, state[y, x - 1], bed[y, x - 1], c, bC)
        FW = f.hllc(self.DIR_W, L, R)[0]
        return FN, FS, FE, FW

    def apply(self, state, bed, dt, t, shared=None):
        """One iteration's tracer on `state` (the iteration's source buffer, not changed); `dt`, `t`: the timestep and time scalars of
        that iteration.  Returns the number of cells moved.  `shared`: a dict in which the species of a TracerSet keep the iteration's
        face fluxes, which depend on the water only."""
        if state.shape != (self.rows, self.cols, 4) or bed.shape != (self.rows, self.cols) or state.dtype != bed.dtype:
            raise ValueError("state must be [rows, cols, 4] and bed [rows, cols], of one dtype")
        if state.dtype.type is not self.real:
            raise ValueError("the face-flux functions and the state differ in precision")
        real = self.real
        dt_real = real(dt)
        dt64, t64 = np.float64(dt_real), np.float64(real(t))
        self.iterations += 1
        M0 = self.M
        # the sources first, in place on the M the step reads
        if dt64 > 0.0:
            flat = M0.reshape(-1)
            for cells, series in self.sources:
                rate = BedShapes.series_fraction(series, t64)
                flat[cells] = self.source_step(flat[cells], rate, dt64, self.dx)
                self.branches["source"].reshape(-1)[cells] += 1
        yy, xx = np.mgrid[0:self.rows, 0:self.cols]
        ring = (xx == 0) | (yy == 0) | (xx == self.cols - 1) | (yy == self.rows - 1)
        self.branches["ring"] += ring
        if not dt_real > 0:
            self.branches["dt_zero"] += ~ring
            return 0
        z, zmax = state[..., 0], state[..., 1]
        disabled = ~ring & ((zmax <= real(-9999.0)) | (z == real(-9999.0)))
        dry = (z - bed) < self.vs                                             # in the state's precision, as the flux kernel tests it
        dry5 = np.zeros_like(dry)
        dry5[1:-1, 1:-1] = dry[1:-1, 1:-1] & dry[2:, 1:-1] & dry[:-2, 1:-1] & dry[1:-1, 2:] & dry[1:-1, :-2]
        dry5 &= ~ring & ~disabled
        moved = ~ring & ~disabled & ~dry5
        self.branches["disabled"] += disabled
        self.branches["dry5"] += dry5
        self.branches["moved"] += moved
        ys, xs = np.nonzero(moved)
        if ys.size == 0:
            self._decay(dt64)
            return 0
        if shared is None or "F" not in shared:
            F = np.array([self.face_fluxes(state, bed, int(x), int(y)) for x, y in zip(xs, ys)], dtype=np.float64).reshape(-1, 4)
            if shared is not None:
                shared["F"] = F
        F = F if shared is None else shared["F"]
        h = z.astype(np.float64) - bed.astype(np.float64)                     # the RAW depth, widened
        c = self.concentration(M0, h)
        out, masks = self.update(M0[ys, xs], c[ys, xs], c[ys + 1, xs], c[ys - 1, xs], c[ys, xs + 1], c[ys, xs - 1],
                                 F[:, 0], F[:, 1], F[:, 2], F[:, 3], dt64, self.dx)
        for name, mask in masks.items():
            self.branches[name][ys, xs] += mask
        shallow = ~(h > self.DEPTH_MIN)
        self.branches["no_concentration"][ys, xs] += shallow[ys, xs] | shallow[ys + 1, xs] | shallow[ys - 1, xs] | shallow[ys, xs + 1] | shallow[ys, xs - 1]
        M1 = M0.copy()
        M1[ys, xs] = out
        self.M = M1
        self._decay(dt64)
        self._exchange(state, bed, ys, xs, dt64, shared)
        return int(ys.size)


class TracerSet:
    """A tracer set on the host (hp_tracer_enable_set restated): K Tracers over one state, each with its own M, sources and decay
    rate.  The device forms the face fluxes once for all of them; here every species is a Tracer of its own, which is the contract."""

    def __init__(self, rows, cols, dx, functions, initial=None, decay=None, species=None, dry_threshold=1e-10, exchange=None, deposit=None, manning=0.0):
        """`exchange`: per species a dict of step 7's parameters or None; `deposit`: per species D0 or None; `manning`: the domain's."""
        said = (([] if species is None else [int(species)]) + ([] if initial is None else [len(initial)]) + ([] if decay is None else [len(decay)]) +
                ([] if exchange is None else [len(exchange)]) + ([] if deposit is None else [len(deposit)]))
        if not said or len(set(said)) != 1 or not 1 <= said[0] <= Tracer.MAX_SPECIES:
            raise ValueError("species, initial and decay must name one number of species, 1..8")
        self.tracers = []
        for s in range(said[0]):
            try:
                self.tracers.append(Tracer(rows, cols, dx, functions, initial=None if initial is None else initial[s], dry_threshold=dry_threshold,
                                           decay=0.0 if decay is None else decay[s], exchange=None if exchange is None else exchange[s],
                                           deposit=None if deposit is None else deposit[s], manning=manning))
            except ValueError as e:
                raise ValueError(f"species {s}: {e}") from None

    def __len__(self):
        return len(self.tracers)

    def __getitem__(self, s):
        return self.tracers[s]

    @property
    def M(self):
        return np.stack([t.M for t in self.tracers])

    @property
    def D(self):
        return np.stack([t.D for t in self.tracers])

    @property
    def iterations(self):
        return self.tracers[0].iterations

    def add_source(self, species, cells, series):
        if not 0 <= species < len(self.tracers):
            raise ValueError(f"species {species} of a tracer of {len(self.tracers)}")
        listed = sum(c.size for t in self.tracers for c, _ in t.sources)
        if sum(len(t.sources) for t in self.tracers) >= Tracer.MAX_SOURCES:
            raise ValueError("more than 64 sources")
        if listed + np.asarray(cells).shape[0] > Tracer.MAX_CELLS:
            raise ValueError("more than 1048576 cells over all sources")
        self.tracers[species].add_source(cells, series)

    def apply(self, state, bed, dt, t):
        shared = {}                                                           # the face fluxes: formed once, as on the device
        return [tr.apply(state, bed, dt, t, shared=shared) for tr in self.tracers][0]

    def branch_totals(self):
        totals = {}
        for tr in self.tracers:
            for k, v in tr.branch_totals().items():
                totals[k] = totals.get(k, 0) + v
        return totals


def tracer_concentration(M, state, bed):
    """The concentration M / h where the depth h = Z - bed exceeds 1e-8 m (the outputs' threshold for a velocity), else -9999."""
    h = np.asarray(state)[..., 0].astype(np.float64) - np.asarray(bed).astype(np.float64)
    wet = h > 1e-8
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(wet, np.asarray(M, dtype=np.float64) / np.where(wet, h, 1.0), -9999.0)


def write_tracer_source_csv(cells_path, series_path, cells, series):
    """The mapFile and the source of a <tracerSource> element: what parse_configuration reads back (repr round-trips every double)."""
    with open(cells_path, "w") as f:
        f.write("x,y\n")
        for x, y in cells:
            f.write(f"{int(x)},{int(y)}\n")
    with open(series_path, "w") as f:
        f.write("time,rate\n")
        for t, r in series:
            f.write(f"{float(t)!r},{float(r)!r}\n")


def write_soil_csv(path, classes):
    """The source of a <soilClasses> element: what parse_configuration reads back (repr round-trips every double)."""
    from . import pack_soil_classes
    with open(path, "w") as f:
        f.write("ks,suction,deficit,capacity\n")
        for c in pack_soil_classes(classes):
            f.write(",".join(repr(float(c[k])) for k in ("ks", "suction", "deficit", "capacity")) + "\n")


def derive_output(what, state, bed, resolution=1.0):
    """Datasets/CRasterDataset.cpp:185-267."""
    code = data_value_code(what)
    z, zmax, qx, qy = (state[..., k].astype(np.float64) for k in range(4))
    bed = bed.astype(np.float64)
    depth = z - bed
    with np.errstate(divide="ignore", invalid="ignore"):
        if code == "depth":
            d = np.maximum(0.0, depth)
            return np.where(d < 1e-8, NODATA, d)
        if code == "maxdepth":
            d = np.maximum(0.0, zmax - bed)
            return np.where((d < 1e-8) | (d <= -9990.0) | (d >= 9999.0), NODATA, d)
        if code == "fsl":
            return np.where((z < bed + 1e-8) | (bed > 9999.0), NODATA, z)
        if code == "maxfsl":
            return np.where((zmax < bed + 1e-8) | (bed > 9999.0), NODATA, zmax)
        if code == "dischargex":
            return qx * resolution
        if code == "dischargey":
            return qy * resolution
        if code == "velocityx":
            return np.where(depth > 1e-8, qx / depth, NODATA)
        if code == "velocityy":
            return np.where(depth > 1e-8, qy / depth, NODATA)
        if code == "froude":
            return np.where(depth > 1e-8, np.sqrt((qx / depth) ** 2 + (qy / depth) ** 2) / np.sqrt(9.81 * depth), NODATA)
    raise ValueError(f"unknown output {what}")


# ------------------------------------------------------------------------------------------------ overviews
AGGREGATES = ("max", "min", "count")                # = hipims_mi.AGG_CODES, in code order


def aggregate_name(aggregate):
    """"max" | "min" | "count" for a name (case-insensitive) or an HP_AGG_* code."""
    if isinstance(aggregate, (int, np.integer)) and not isinstance(aggregate, bool) and 0 <= int(aggregate) < len(AGGREGATES):
        return AGGREGATES[int(aggregate)]
    if isinstance(aggregate, str) and aggregate.lower() in AGGREGATES:
        return aggregate.lower()
    raise ValueError(f"unknown aggregate {aggregate}")


def _order_keys(a):
    """The elements of a float64 / float32 array in their own order as unsigned integers of the same width (csrc/hp_overview.hpp:
    overview_key): negative values complemented, the others with the sign bit set; -0.0 lies below +0.0.  Elements that do not take
    part -- NODATA and NaN -- get 0, which lies below every key."""
    a = np.ascontiguousarray(a)
    if a.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
        a = a.astype(np.float64)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    bits = a.view(u)
    top = u(1) << u(8 * a.itemsize - 1)
    keys = np.where(bits & top != 0, ~bits, bits | top)
    return np.where((a != NODATA) & ~np.isnan(a), keys, u(0)), a.dtype


def _from_keys(keys, dtype, complemented=False):
    """The values of _order_keys' keys (their complements with complemented=True); NODATA where the key is 0."""
    u = keys.dtype.type
    top = u(1) << u(8 * keys.itemsize - 1)
    k = ~keys if complemented else keys
    values = np.where(k & top != 0, k ^ top, ~k).view(dtype)
    return np.where(keys == 0, dtype.type(NODATA), values)


def overview(raster, factor, aggregate, row_offset=0):
    """hp_domain_overview in NumPy: `raster` is a full-resolution raster as derive_output delivers it, [nrows, cols] with row 0 =
    row `row_offset` of the global grid; the result is float64 [block_rows, block_cols] over blocks of factor x factor cells
    anchored to that grid (hipims_mi.overview_shape), edge blocks partial.  A cell takes part iff its value is neither NODATA nor
    NaN; "max" / "min": the largest / smallest participating value (NODATA if none; -0.0 below +0.0), "count": their number."""
    from . import overview_shape
    kind = aggregate_name(aggregate)
    a = np.asarray(raster)
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError("the raster must be [rows, cols]")
    a = a.astype(np.float64)
    nrows, cols = a.shape
    first, brows, bcols = overview_shape(cols, factor, row_offset, 0, nrows)
    if nrows == 0:
        return np.empty((0, bcols), np.float64)
    # where the blocks start, as indices into the raster (the first block row may start below the raster's row 0)
    row_cuts = np.maximum(0, np.arange(first, first + brows) * int(factor) - int(row_offset))
    col_cuts = np.arange(bcols) * int(factor)
    keys, dtype = _order_keys(a)
    if kind == "count":
        part = (keys != 0).astype(np.int64)
        return np.add.reduceat(np.add.reduceat(part, row_cuts, axis=0), col_cuts, axis=1).astype(np.float64)
    if kind == "min":
        keys = np.where(keys != 0, ~keys, np.uint64(0))
    folded = np.maximum.reduceat(np.maximum.reduceat(keys, row_cuts, axis=0), col_cuts, axis=1)
    return _from_keys(folded, dtype, complemented=kind == "min")


def combine_overviews(parts, aggregate):
    """The overview of a row range from those of its parts, each a (first_block_row, array[block_rows, block_cols]) pair laid on the
    global block grid (None entries are skipped); a block that two parts touch -- a cut inside a block -- gets the larger / smaller
    of its two values, ignoring NODATA, or the sum of its two counts.  -> (first_block_row, array) over the block rows the parts
    span; block rows that no part touches hold NODATA (0 for counts).  Order-independent like the device's own fold: equal to the
    uncut overview in every bit, whatever the cut."""
    kind = aggregate_name(aggregate)
    parts = [(int(f), np.asarray(a)) for f, a in (p for p in parts if p is not None)]
    if not parts:
        raise ValueError("no part")
    dtype, bcols = parts[0][1].dtype, parts[0][1].shape[1]
    if any(a.ndim != 2 or a.dtype != dtype or a.shape[1] != bcols for _, a in parts):
        raise ValueError("the parts' overviews differ in type or block columns")
    lo, hi = min(f for f, _ in parts), max(f + len(a) for f, a in parts)
    if kind == "count":
        out = np.zeros((hi - lo, bcols), dtype)
        for f, a in parts:
            out[f - lo:f - lo + len(a)] += a
        return lo, out
    keys0, kdtype = _order_keys(np.zeros((1, 1), dtype))
    folded = np.zeros((hi - lo, bcols), keys0.dtype)
    for f, a in parts:
        keys, _ = _order_keys(a)
        if kind == "min":
            keys = np.where(keys != 0, ~keys, keys.dtype.type(0))
        folded[f - lo:f - lo + len(a)] = np.maximum(folded[f - lo:f - lo + len(a)], keys)
    return lo, _from_keys(folded, kdtype, complemented=kind == "min")


# ------------------------------------------------------------------------------------------------ selected cells (CSR)
def sparse(rasters, select_raster, above):
    """hp_domain_sparse in NumPy: `rasters` are full-resolution rasters [nrows, cols] as derive_output delivers them (or those
    rounded to float32), `select_raster` the float64 raster of the selecting value.  A cell is selected iff its selecting value v
    satisfies v != NODATA and v > above (a NaN fails).  -> (row_ptr uint64 [nrows + 1], col uint32 [selected], [the rasters' values
    at the selected cells, in their own type]), entries ascending by (row, column)."""
    sel = np.asarray(select_raster, np.float64)
    if sel.ndim != 2:
        raise ValueError("the select raster must be [rows, cols]")
    if np.isnan(above):
        raise ValueError("above is a NaN")
    rasters = [np.asarray(a) for a in rasters]
    if any(a.shape != sel.shape for a in rasters):
        raise ValueError("the rasters differ in shape from the select raster")
    with np.errstate(invalid="ignore"):
        chosen = (sel != NODATA) & (sel > above)
    row_ptr = np.zeros(sel.shape[0] + 1, np.uint64)
    row_ptr[1:] = np.cumsum(chosen.sum(axis=1, dtype=np.uint64), dtype=np.uint64)
    rows, cols = np.nonzero(chosen)                   # (row-major: ascending by row, then column)
    return row_ptr, cols.astype(np.uint32), [a[rows, cols] for a in rasters]


def combine_sparse(parts):
    """The (row_ptr, col, values) results of consecutive row ranges, south to north, as the result of the whole range: the entries
    concatenated, each part's row_ptr shifted by the entries in front of it."""
    parts = list(parts)
    if not parts:
        raise ValueError("no part")
    if any(len(p[2]) != len(parts[0][2]) for p in parts):
        raise ValueError("the parts differ in their number of values")
    row_ptrs, shift = [np.zeros(1, np.uint64)], np.uint64(0)
    for row_ptr, _, _ in parts:
        row_ptr = np.asarray(row_ptr, np.uint64)
        row_ptrs.append(row_ptr[1:] + shift)
        shift = shift + row_ptr[-1]
    return (np.concatenate(row_ptrs), np.concatenate([np.asarray(p[1], np.uint32) for p in parts]),
            [np.concatenate([p[2][k] for p in parts]) for k in range(len(parts[0][2]))])


def sparse_to_dense(row_ptr, col, values, cols, fill=NODATA):
    """The raster [len(row_ptr) - 1, cols] that holds `values` at the entries of (row_ptr, col) and `fill` elsewhere."""
    row_ptr, col, values = np.asarray(row_ptr, np.uint64), np.asarray(col), np.asarray(values)
    out = np.full((len(row_ptr) - 1, int(cols)), fill, values.dtype)
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr.astype(np.int64)))
    out[rows, col.astype(np.int64)] = values
    return out


def run_model(xml_path, make_sim=None, batch=None, output_format=".npy", max_outputs=None, log=None):
    """CModel::runModel for one domain (see model.py): advance to each output time, write the configured rasters
    there.  `batch` fixes the batch size (the reference's `queueMode="fixed"`); default = the autotuner.
    make_sim(cfg, cols, rows, res) may return any object with the Domain surface (the tests pass the oracle);
    the default is the HIP engine.  Returns [(time, {value: south-up array})]."""
    from .model import Model
    m = Model(xml_path, make_sim=make_sim, output_format=output_format, log=log)
    if batch:
        m.scheme.automatic_queue = False
        m.scheme.queue_addition_size = int(batch)
    try:
        return m.run(max_outputs=max_outputs)
    finally:
        m.close()
