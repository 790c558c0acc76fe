"""hipims_mi -- thin ctypes binding of ``libhipims_mi.so`` (the C ABI in ``include/hipims_mi.h``).

This is the Python face of the drop-in boundary used by the tests and ``bench.py``; the product is the
shared library.  There is no CPU fallback anywhere in this package: loading fails loudly when the
library is missing, and creating a domain fails when no HIP device is usable.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(PKG_ROOT, "lib", "libhipims_mi.so")

# enums of include/hipims_mi.h
SCHEME_GODUNOV, SCHEME_MUSCL_HANCOCK, SCHEME_INERTIAL = 0, 1, 2
ARRAY_STATE, ARRAY_BED, ARRAY_MANNING = 0, 1, 2
QUIRK_CFL_READS_PRIMARY, QUIRK_BDY_TRUNCATED, QUIRK_MUSCL_NEIGHBOUR_Y_IS_BED, QUIRKS_REFERENCE = 1, 2, 4, 7
MATH_FAST, MATH_STRICT = 0, 1
KERNEL_AUTO, KERNEL_BASIC = 0, 1
UNIFORM_RAIN_INTENSITY, UNIFORM_LOSS_RATE = 0, 1
GRIDDED_RAIN_INTENSITY, GRIDDED_RAIN_ACCUMUL, GRIDDED_MASS_FLUX = 0, 1, 2
DEPTH_IGNORE, DEPTH_IS_FSL, DEPTH_IS_DEPTH, DEPTH_IS_CRITICAL = 0, 1, 2, 3
DISCHARGE_IGNORE, DISCHARGE_IS_DISCHARGE, DISCHARGE_IS_VELOCITY, DISCHARGE_IS_VOLUME = 0, 1, 2, 3
PTR_STATE_NEXT_SRC, PTR_STATE_OTHER, PTR_BED, PTR_MANNING, PTR_CFL_MAX, PTR_SCALARS = range(6)
(OUT_DEPTH, OUT_MAXDEPTH, OUT_FSL, OUT_MAXFSL, OUT_DISCHARGE_X, OUT_DISCHARGE_Y, OUT_VELOCITY_X, OUT_VELOCITY_Y, OUT_FROUDE,
 OUT_COUNT) = range(10)
# the front end's value names (frontend.data_value_code) -> HP_OUT_*
OUT_CODES = {"depth": OUT_DEPTH, "maxdepth": OUT_MAXDEPTH, "fsl": OUT_FSL, "maxfsl": OUT_MAXFSL, "dischargex": OUT_DISCHARGE_X,
             "dischargey": OUT_DISCHARGE_Y, "velocityx": OUT_VELOCITY_X, "velocityy": OUT_VELOCITY_Y, "froude": OUT_FROUDE}
AGG_MAX, AGG_MIN, AGG_COUNT, AGG_KINDS = range(4)
# the aggregates' names (a <dataTarget>'s aggregate attribute) -> HP_AGG_*
AGG_CODES = {"max": AGG_MAX, "min": AGG_MIN, "count": AGG_COUNT}
OVERVIEW_FACTOR_MAX = 4096
(PEAK_SPEED, PEAK_UNIT_DISCHARGE, PEAK_HAZARD, PEAK_ARRIVAL_TIME, PEAK_WET_DURATION, PEAK_COUNT) = range(6)
# the front end's peak value names (frontend.peak_value_code) -> HP_PEAK_*
PEAK_CODES = {"peakspeed": PEAK_SPEED, "peakunitdischarge": PEAK_UNIT_DISCHARGE, "hazard": PEAK_HAZARD,
              "arrivaltime": PEAK_ARRIVAL_TIME, "wetduration": PEAK_WET_DURATION}
NO_CELL = 2 ** 64 - 1          # hp_domain_stats_t: "no such cell"

EXPORTS = [
    "hp_abi_version", "hp_device_count", "hp_device_info", "hp_last_error", "hp_set_log_sink", "hp_domain_desc_default",
    "hp_domain_create", "hp_domain_destroy", "hp_domain_upload", "hp_domain_download", "hp_domain_upload_rows", "hp_state_save", "hp_state_restore",
    "hp_domain_derive", "hp_domain_stats", "hp_overview_shape", "hp_domain_overview", "hp_domain_sparse",
    "hp_peaks_enable", "hp_peaks_disable", "hp_peaks_reset", "hp_peaks_sample", "hp_peaks_read", "hp_peaks_info",
    "hp_probes_enable", "hp_probes_disable", "hp_probes_reset", "hp_probes_sample", "hp_probes_read", "hp_probes_info",
    "hp_zones_enable", "hp_zones_disable", "hp_zones_reset", "hp_zones_sample", "hp_zones_read", "hp_zones_info",
    "hp_bed_shape_add", "hp_bed_shapes_clear", "hp_bed_apply", "hp_bed_info",
    "hp_boundary_add_uniform", "hp_boundary_add_gridded", "hp_boundary_add_cell", "hp_boundary_add_links", "hp_links_read", "hp_links_info",
    "hp_boundary_add_infiltration", "hp_infiltration_read", "hp_infiltration_info", "hp_boundary_add_open", "hp_open_read", "hp_open_info", "hp_boundary_clear", "hp_boundaries_fused",
    "hp_tracer_enable", "hp_tracer_disable", "hp_tracer_add_source", "hp_tracer_sources_clear", "hp_tracer_read", "hp_tracer_write", "hp_tracer_info",
    "hp_tracer_enable_set", "hp_tracer_add_source_to", "hp_tracer_read_species", "hp_tracer_write_species", "hp_tracer_set_info",
    "hp_tracer_set_exchange", "hp_tracer_deposit_read", "hp_tracer_deposit_write", "hp_tracer_exchange_info", "hp_set_target_time", "hp_set_time",
    "hp_force_timestep", "hp_reset_counters", "hp_update_timestep", "hp_step_batch", "hp_read_scalars",
    "hp_sync", "hp_is_busy", "hp_step_begin", "hp_step_end", "hp_step_needs_reduction", "hp_device_ptr", "hp_stream", "hp_set_halo_overlap",
    "hp_stream_halo", "hp_comm_load", "hp_comm_unique_id", "hp_strip_comm_init", "hp_strip_step_batch", "hp_strip_update_timestep",
    "hp_strip_comm_destroy", "hp_strip_info", "hp_strip_peer_ticket", "hp_strip_peer_connect", "hp_strip_peer_round",
    "hp_strip_peer_disconnect", "hp_timer_start",
    "hp_timer_stop", "hp_kernel_timing", "hp_kernel_timing_read", "hp_kernel_timing_overhead",
    "hp_launch_counts", "hp_pair_stats", "hp_pair_wall_stats",
]


class HipimsError(RuntimeError):
    pass


LOG_SINK = C.CFUNCTYPE(None, C.c_int, C.c_char_p, C.c_void_p)     # hp_log_sink_t
_log_sink_ref = None


def set_log_sink(callback):
    """Route every failing call's message to `callback(level, text)` (the reference's model::doError ->
    CLog::writeError place, main.cpp:631-652).  None removes the sink."""
    global _log_sink_ref
    lib = load_library()
    if callback is None:
        sink = C.cast(None, LOG_SINK)
    else:
        sink = LOG_SINK(lambda level, msg, _user: callback(int(level), msg.decode(errors="replace")))
    _check(lib, lib.hp_set_log_sink(sink, None), "hp_set_log_sink")
    _log_sink_ref = sink          # keep the trampoline alive while the library may call it


class DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("arch", C.c_char * 32), ("compute_units", C.c_int32),
                ("clock_mhz", C.c_int32), ("global_mem_bytes", C.c_uint64), ("lds_bytes_per_cu", C.c_uint64),
                ("wavefront", C.c_int32), ("fp64", C.c_int32)]


class DomainDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("cols", C.c_int64), ("rows", C.c_int64),
                ("dx", C.c_double), ("precision", C.c_int32), ("scheme", C.c_int32), ("courant", C.c_double),
                ("dry_threshold", C.c_double), ("friction", C.c_int32), ("dynamic_dt", C.c_int32),
                ("dt_fixed", C.c_double), ("dt_initial", C.c_double), ("t_end", C.c_double),
                ("quirks", C.c_uint32), ("math_mode", C.c_int32), ("kernel", C.c_int32),
                ("global_rows", C.c_int64), ("row_offset", C.c_int64), ("ghost_rows", C.c_int32), ("reserved0", C.c_int32)]


class StripInfo(C.Structure):
    _fields_ = [("library", C.c_char * 256), ("comm_ranks", C.c_int32), ("comm_rank", C.c_int32),
                ("halo_overlap", C.c_int32), ("ghost_rows", C.c_int32), ("peer_max", C.c_int32), ("peer_halo", C.c_int32)]


class ScalarsOut(C.Structure):
    _fields_ = [("time", C.c_double), ("timestep", C.c_double), ("time_hydrological", C.c_double),
                ("time_target", C.c_double), ("batch_timesteps", C.c_double), ("batch_successful", C.c_uint32),
                ("batch_skipped", C.c_uint32), ("cells_calculated", C.c_uint64), ("iterations", C.c_uint64)]


class DomainStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("cells", C.c_uint64), ("cells_wet", C.c_uint64),
                ("volume", C.c_double), ("max_depth", C.c_double), ("max_speed", C.c_double),
                ("max_depth_cell", C.c_uint64), ("max_speed_cell", C.c_uint64)]


class PeaksDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("values_mask", C.c_uint32), ("arrival_depth", C.c_double)]


class ProbesDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("capacity", C.c_uint32), ("gauge_count", C.c_uint64),
                ("gauge_cells", C.POINTER(C.c_uint64)), ("section_count", C.c_uint32),
                ("section_offsets", C.POINTER(C.c_uint64)), ("section_cells", C.POINTER(C.c_uint64)),
                ("section_wx", C.POINTER(C.c_int8)), ("section_wy", C.POINTER(C.c_int8))]


class ZonesDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("capacity", C.c_uint32), ("zone_count", C.c_uint32), ("reserved", C.c_uint32),
                ("zone_of_cell", C.POINTER(C.c_uint16)), ("flood_depth", C.c_double)]


class BedShapeDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("series_entries", C.c_uint32), ("cell_count", C.c_uint64),
                ("cells", C.POINTER(C.c_uint64)), ("target", C.POINTER(C.c_double)), ("series", C.POINTER(C.c_double))]


class BedInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("shapes", C.c_uint32), ("cells_local", C.c_uint64), ("applies", C.c_uint64),
                ("changed_last", C.c_uint64), ("changed_total", C.c_uint64), ("t_last", C.c_double)]


LINK_WEIR, LINK_ORIFICE, LINK_PUMP = 0, 1, 2         # HP_LINK_*
LINK_KINDS = {"weir": LINK_WEIR, "orifice": LINK_ORIFICE, "culvert": LINK_ORIFICE, "pump": LINK_PUMP}
# hp_link_t and hp_link_record_t as NumPy records: arrays of them go through the ABI as they are
LINK_DTYPE = np.dtype([("cell_a", np.uint64), ("cell_b", np.uint64), ("kind", np.int32), ("one_way", np.int32),
                       ("level", np.float64), ("size", np.float64), ("coeff", np.float64), ("limit", np.float64)])
LINK_RECORD_DTYPE = np.dtype([("q_last", np.float64), ("volume", np.float64), ("active", np.uint64), ("reserved", np.uint64)])


def pack_links(links, cols):
    """Links as an array of LINK_DTYPE.  `links`: such an array, or a sequence of dicts / tuples (a, b, kind, one_way, level, size,
    coeff, limit) where a and b are flat ids y * cols + x of the GLOBAL grid or (x, y) pairs and kind an HP_LINK_* code or its name;
    one_way defaults to 0, coeff to 0 and limit to +inf for an orifice, 0 otherwise."""
    if isinstance(links, np.ndarray) and links.dtype == LINK_DTYPE:
        return np.ascontiguousarray(links).reshape(-1)
    names = ("a", "b", "kind", "one_way", "level", "size", "coeff", "limit")
    out = np.zeros(len(links), LINK_DTYPE)

    def cell(c):
        if np.ndim(c) == 0:
            return int(c)
        x, y = int(c[0]), int(c[1])
        if not (0 <= x < cols and y >= 0):
            raise ValueError("a link's cell lies outside the grid")
        return y * cols + x
    for k, l in enumerate(links):
        l = dict(l) if isinstance(l, dict) else dict(zip(names, l))
        kind = l["kind"]
        kind = LINK_KINDS[kind.lower()] if isinstance(kind, str) else int(kind)
        out[k] = (cell(l["a"]), cell(l["b"]), kind, int(l.get("one_way", 0)), float(l["level"]), float(l["size"]), float(l.get("coeff", 0.0)),
                  float(l.get("limit", np.inf if kind == LINK_ORIFICE else 0.0)))
    return out


EDGE_SOUTH, EDGE_NORTH, EDGE_WEST, EDGE_EAST = 0, 1, 2, 3      # HP_EDGE_*
EDGES = {"south": EDGE_SOUTH, "north": EDGE_NORTH, "west": EDGE_WEST, "east": EDGE_EAST}
# hp_open_segment_t and hp_open_record_t as NumPy records: arrays of them go through the ABI as they are
OPEN_SEGMENT_DTYPE = np.dtype([("edge", np.int32), ("reserved", np.int32), ("first", np.int64), ("last", np.int64)])
OPEN_RECORD_DTYPE = np.dtype([("q_last", np.float64), ("volume", np.float64), ("active", np.uint64), ("reserved", np.uint64)])


def pack_open_segments(segments, cols, global_rows):
    """Segments of the edge ring as an array of OPEN_SEGMENT_DTYPE.  `segments`: such an array, or a sequence of dicts(edge, first, last)
    / tuples (edge, first, last) / bare edges, where an edge is an HP_EDGE_* code or its name; first and last are GLOBAL indices along the
    edge (the column for south and north, the row for west and east), inclusive, and default to the whole edge without its corners."""
    if isinstance(segments, np.ndarray) and segments.dtype == OPEN_SEGMENT_DTYPE:
        return np.ascontiguousarray(segments).reshape(-1)
    if isinstance(segments, (str, int, np.integer, dict)):
        segments = [segments]
    out = np.zeros(len(segments), OPEN_SEGMENT_DTYPE)
    for k, s in enumerate(segments):
        if isinstance(s, (str, int, np.integer)):
            s = dict(edge=s)
        s = dict(s) if isinstance(s, dict) else dict(zip(("edge", "first", "last"), s))
        edge = s["edge"]
        if isinstance(edge, str):
            if edge.lower() not in EDGES:
                raise ValueError(f"segment {k}: unknown edge {edge!r}")
            edge = EDGES[edge.lower()]
        n = int(cols) if int(edge) in (EDGE_SOUTH, EDGE_NORTH) else int(global_rows)
        first = 1 if s.get("first") is None else int(s["first"])
        last = n - 2 if s.get("last") is None else int(s["last"])
        out[k] = (int(edge), int(s.get("reserved", 0)), first, last)
    return out


# hp_soil_class_t as a NumPy record, and hp_infiltration_desc_t
SOIL_CLASS_DTYPE = np.dtype([("ks", np.float64), ("suction", np.float64), ("deficit", np.float64), ("capacity", np.float64)])


class InfiltrationDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("class_count", C.c_uint32), ("classes", C.c_void_p), ("soil_of_cell", C.c_void_p),
                ("initial", C.c_void_p)]


def pack_soil_classes(classes):
    """Soil classes as an array of SOIL_CLASS_DTYPE.  `classes`: such an array, or a sequence of dicts / tuples (ks, suction,
    deficit, capacity); capacity defaults to +inf.  Class k of the id raster is entry k - 1."""
    if isinstance(classes, np.ndarray) and classes.dtype == SOIL_CLASS_DTYPE:
        return np.ascontiguousarray(classes).reshape(-1)
    names = ("ks", "suction", "deficit", "capacity")
    out = np.zeros(len(classes), SOIL_CLASS_DTYPE)
    for k, c in enumerate(classes):
        c = dict(c) if isinstance(c, dict) else dict(zip(names, c))
        out[k] = (float(c["ks"]), float(c["suction"]), float(c["deficit"]), float(c.get("capacity", np.inf)))
    return out


def soil_ids(values, what="the soil raster"):
    """A raster of soil class ids as uint8: every value an integer in 0..255 (0 = impervious), else ValueError."""
    v = np.asarray(values)
    if v.dtype.kind not in "iu":
        if not np.isfinite(v).all() or (v != np.floor(v)).any():
            raise ValueError(f"{what}: soil class ids must be integers")
    if v.size and (v.min() < 0 or v.max() > 255):
        raise ValueError(f"{what}: soil class ids must lie in 0..255")
    return np.ascontiguousarray(v.astype(np.uint8))


# hp_tracer_desc_t
class TracerDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("initial", C.c_void_p)]


TRACER_MAX_SPECIES = 8


# hp_tracer_set_desc_t
class TracerSetDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("species", C.c_uint32), ("decay", C.c_void_p), ("initial", C.c_void_p)]


# hp_tracer_exchange_desc_t
class TracerExchangeDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("species", C.c_uint32), ("settling", C.c_double), ("tau_deposit", C.c_double),
                ("tau_erode", C.c_double), ("erodibility", C.c_double), ("deposit_initial", C.c_void_p)]


_lib = None


def load_library(path: str | None = None):
    """dlopen libhipims_mi.so (no GPU needed for this) and declare the signatures."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("HIPIMS_MI_LIB") or LIB_PATH       # HIPIMS_MI_LIB: kernel-variant experiments
    # One HIP runtime per process.  torch wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's): if
    # torch initialises AFTER this library has pulled in the system runtime, the process ends up with two
    # runtimes and torch sees no GPU.  Loading torch first makes the dynamic loader bind this library to torch's
    # copy, so device pointers and streams can be shared with torch.distributed (RCCL).  Set
    # HIPIMS_MI_NO_TORCH=1 for a torch-free process (then the system runtime is used).
    if os.environ.get("HIPIMS_MI_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(path):
        raise HipimsError(f"{path} is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"(make -C hipims-ocl_amd/csrc); there is no CPU fallback")
    lib = C.CDLL(path)
    lib.hp_last_error.restype = C.c_char_p
    lib.hp_set_log_sink.argtypes = [LOG_SINK, C.c_void_p]
    lib.hp_domain_desc_default.restype = None
    lib.hp_domain_desc_default.argtypes = [C.POINTER(DomainDesc)]
    lib.hp_domain_create.argtypes = [C.POINTER(DomainDesc), C.POINTER(C.c_void_p)]
    lib.hp_domain_destroy.argtypes = [C.c_void_p]
    lib.hp_domain_upload.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    lib.hp_domain_download.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64]
    lib.hp_domain_upload_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
    if hasattr(lib, "hp_domain_derive"):                # (absent from older builds loaded through HIPIMS_MI_LIB for A/B runs: calling it there raises)
        lib.hp_domain_derive.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int64, C.c_int64]
        lib.hp_domain_stats.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(DomainStats)]
    if hasattr(lib, "hp_domain_overview"):              # (absent from older builds, as above)
        lib.hp_overview_shape.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.hp_domain_overview.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                           C.c_int64, C.c_int64]
    if hasattr(lib, "hp_domain_sparse"):                # (absent from older builds, as above)
        lib.hp_domain_sparse.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.c_int64, C.c_int64]
    if hasattr(lib, "hp_peaks_enable"):                 # (absent from older builds, as above)
        lib.hp_peaks_enable.argtypes = [C.c_void_p, C.POINTER(PeaksDesc)]
        lib.hp_peaks_disable.argtypes = [C.c_void_p]
        lib.hp_peaks_reset.argtypes = [C.c_void_p]
        lib.hp_peaks_sample.argtypes = [C.c_void_p]
        lib.hp_peaks_read.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int64, C.c_int64]
        lib.hp_peaks_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(lib, "hp_probes_enable"):                # (absent from older builds, as above)
        lib.hp_probes_enable.argtypes = [C.c_void_p, C.POINTER(ProbesDesc)]
        lib.hp_probes_disable.argtypes = [C.c_void_p]
        lib.hp_probes_reset.argtypes = [C.c_void_p]
        lib.hp_probes_sample.argtypes = [C.c_void_p]
        lib.hp_probes_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_double)]
        lib.hp_probes_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if hasattr(lib, "hp_zones_enable"):                 # (absent from older builds, as above)
        lib.hp_zones_enable.argtypes = [C.c_void_p, C.POINTER(ZonesDesc)]
        lib.hp_zones_disable.argtypes = [C.c_void_p]
        lib.hp_zones_reset.argtypes = [C.c_void_p]
        lib.hp_zones_sample.argtypes = [C.c_void_p]
        lib.hp_zones_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.hp_zones_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if hasattr(lib, "hp_bed_shape_add"):                # (absent from older builds, as above)
        lib.hp_bed_shape_add.argtypes = [C.c_void_p, C.POINTER(BedShapeDesc)]
        lib.hp_bed_shapes_clear.argtypes = [C.c_void_p]
        lib.hp_bed_apply.argtypes = [C.c_void_p]
        lib.hp_bed_info.argtypes = [C.c_void_p, C.POINTER(BedInfo)]
    if hasattr(lib, "hp_boundary_add_links"):           # (absent from older builds, as above)
        lib.hp_boundary_add_links.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        lib.hp_links_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        lib.hp_links_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if hasattr(lib, "hp_boundary_add_infiltration"):    # (absent from older builds, as above)
        lib.hp_boundary_add_infiltration.argtypes = [C.c_void_p, C.POINTER(InfiltrationDesc)]
        lib.hp_infiltration_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
        lib.hp_infiltration_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    if hasattr(lib, "hp_boundary_add_open"):            # (absent from older builds, as above)
        lib.hp_boundary_add_open.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        lib.hp_open_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        lib.hp_open_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    if hasattr(lib, "hp_tracer_enable"):                # (absent from older builds, as above)
        lib.hp_tracer_enable.argtypes = [C.c_void_p, C.POINTER(TracerDesc)]
        lib.hp_tracer_disable.argtypes = [C.c_void_p]
        lib.hp_tracer_add_source.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
        lib.hp_tracer_sources_clear.argtypes = [C.c_void_p]
        lib.hp_tracer_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
        lib.hp_tracer_write.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
        lib.hp_tracer_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    if hasattr(lib, "hp_tracer_enable_set"):
        lib.hp_tracer_enable_set.argtypes = [C.c_void_p, C.POINTER(TracerSetDesc)]
        lib.hp_tracer_add_source_to.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
        lib.hp_tracer_read_species.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64]
        lib.hp_tracer_write_species.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64]
        lib.hp_tracer_set_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    if hasattr(lib, "hp_tracer_set_exchange"):
        lib.hp_tracer_set_exchange.argtypes = [C.c_void_p, C.POINTER(TracerExchangeDesc)]
        lib.hp_tracer_deposit_read.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64]
        lib.hp_tracer_deposit_write.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_int64]
        lib.hp_tracer_exchange_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(TracerExchangeDesc)]
    lib.hp_state_save.argtypes = [C.c_void_p]
    lib.hp_state_restore.argtypes = [C.c_void_p]
    lib.hp_boundary_add_uniform.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_double, C.c_double]
    lib.hp_boundary_add_gridded.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                            C.c_double, C.c_double, C.c_double, C.c_double]
    lib.hp_boundary_add_cell.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                         C.c_double, C.c_double]
    lib.hp_boundary_clear.argtypes = [C.c_void_p]
    lib.hp_boundaries_fused.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.hp_set_target_time.argtypes = [C.c_void_p, C.c_double]
    lib.hp_force_timestep.argtypes = [C.c_void_p, C.c_double]
    lib.hp_set_time.argtypes = [C.c_void_p, C.c_double]
    lib.hp_reset_counters.argtypes = [C.c_void_p]
    lib.hp_update_timestep.argtypes = [C.c_void_p]
    lib.hp_step_batch.argtypes = [C.c_void_p, C.c_uint32]
    lib.hp_read_scalars.argtypes = [C.c_void_p, C.POINTER(ScalarsOut)]
    lib.hp_sync.argtypes = [C.c_void_p]
    lib.hp_is_busy.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.hp_step_begin.argtypes = [C.c_void_p]
    lib.hp_step_end.argtypes = [C.c_void_p]
    lib.hp_step_needs_reduction.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.hp_device_ptr.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.hp_stream.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.hp_set_halo_overlap.argtypes = [C.c_void_p, C.c_int]
    lib.hp_stream_halo.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.hp_comm_load.argtypes = [C.c_char_p]
    lib.hp_comm_unique_id.argtypes = [C.c_void_p]
    lib.hp_strip_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.hp_strip_step_batch.argtypes = [C.c_void_p, C.c_uint32]
    lib.hp_strip_update_timestep.argtypes = [C.c_void_p]
    lib.hp_strip_comm_destroy.argtypes = [C.c_void_p]
    lib.hp_strip_info.argtypes = [C.c_void_p, C.POINTER(StripInfo)]
    lib.hp_strip_peer_ticket.argtypes = [C.c_void_p, C.c_void_p]
    lib.hp_strip_peer_connect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.hp_strip_peer_round.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_double)]
    lib.hp_strip_peer_disconnect.argtypes = [C.c_void_p]
    lib.hp_timer_start.argtypes = [C.c_void_p]
    lib.hp_timer_stop.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.hp_kernel_timing.argtypes = [C.c_void_p, C.c_int]
    lib.hp_kernel_timing_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    if hasattr(lib, "hp_kernel_timing_overhead"):       # (absent from round-3 builds loaded through HIPIMS_MI_LIB for A/B runs)
        lib.hp_kernel_timing_overhead.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    if hasattr(lib, "hp_launch_counts"):                # (absent from builds before round 5, as above)
        lib.hp_launch_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.hp_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.hp_device_info.argtypes = [C.c_int, C.POINTER(DeviceInfo)]
    _lib = lib
    return lib


def _check(lib, rc, what):
    if rc != 0:
        raise HipimsError(f"{what} failed ({rc}): {lib.hp_last_error().decode(errors='replace')}")


def split_probe_records(records, gauges, sections):
    """[n, 1 + 4 G + S] probe records (hp_probes_read's layout) as {"t": [n], "gauges": [n, G, 4], "sections": [n, S]}."""
    rec = np.asarray(records, dtype=np.float64).reshape(-1, 1 + 4 * gauges + sections)
    return dict(t=rec[:, 0].copy(), gauges=rec[:, 1:1 + 4 * gauges].reshape(-1, gauges, 4).copy(), sections=rec[:, 1 + 4 * gauges:].copy())


def overview_shape(cols, factor, row_offset=0, row0=0, nrows=0):
    """hp_overview_shape's arithmetic: (first_block_row, block_rows, block_cols) of rows [row0, row0 + nrows) of a local array of
    `cols` columns whose row 0 is row `row_offset` of the global grid, in blocks of factor x factor cells anchored to that grid."""
    cols, factor, lo, nrows = int(cols), int(factor), int(row_offset) + int(row0), int(nrows)
    if not 1 <= factor <= OVERVIEW_FACTOR_MAX:
        raise ValueError("factor outside 1..4096")
    if cols < 1 or lo < 0 or nrows < 0:
        raise ValueError("row range out of bounds")
    first = lo // factor
    return first, (0 if nrows == 0 else (lo + nrows - 1) // factor - first + 1), -(-cols // factor)


def overview_pairs(values, aggregates):
    """The (value, aggregate) pairs of Domain.overview as HP_OUT_* / HP_AGG_* codes: `values` are the front end's value names
    (frontend.data_value_code) or codes, `aggregates` names of AGG_CODES or codes -- one per value, or one for all of them."""
    from .frontend import data_value_code
    values = [values] if isinstance(values, (str, int)) else list(values)
    aggregates = [aggregates] * len(values) if isinstance(aggregates, (str, int)) else list(aggregates)
    if len(aggregates) != len(values):
        raise ValueError("one aggregate per value, or one for all of them")
    pairs = []
    for v, a in zip(values, aggregates):
        vc = v if isinstance(v, int) else OUT_CODES.get(data_value_code(v))
        ac = a if isinstance(a, int) else AGG_CODES.get(str(a).lower())
        if vc is None or not 0 <= vc < OUT_COUNT:
            raise ValueError(f"unknown output {v}")
        if ac is None or not 0 <= ac < AGG_KINDS:
            raise ValueError(f"unknown aggregate {a}")
        if (vc, ac) in pairs:
            raise ValueError(f"the pair ({v}, {a}) is listed twice")
        pairs.append((vc, ac))
    return pairs


ZONE_WORDS = 7                 # HP_ZONE_WORDS: cells, wet, flooded, depth_hi, depth_lo, max_depth, max_speed
ZONES_MAX = 4096


def split_zone_records(records, zone_count, dx):
    """[n, 1 + 7 Z] zone records of uint64 words (hp_zones_read's layout) as {"t": [n], "cells" | "wet" | "flooded" | "depth_hi" |
    "depth_lo": uint64 [n, Z], "volume" | "max_depth" | "max_speed": float64 [n, Z]}.  The volume comes from the exact integer
    S = depth_hi * 2^32 + depth_lo with one rounding (what Python's int / int gives), times dx * dx."""
    rec = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 1 + ZONE_WORDS * zone_count)
    z = rec[:, 1:].reshape(-1, zone_count, ZONE_WORDS)
    out = dict(t=rec[:, 0].copy().view(np.float64))
    for k, name in enumerate(("cells", "wet", "flooded", "depth_hi", "depth_lo")):
        out[name] = z[:, :, k].copy()
    # S with its limbs normalised: lo < 2^32 and hi < 2^53 are both exact in fp64, and so is hi * 2^32, which leaves the one
    # addition as the only rounding (the correctly rounded S); dividing by 2^32 is exact.  Whole arrays at a time: a full buffer
    # of 4096 zones is some millions of entries.
    hi = out["depth_hi"] + (out["depth_lo"] >> np.uint64(32))
    lo = out["depth_lo"] & np.uint64(0xffffffff)
    if hi.size and int(hi.max()) >> 53:                 # (2^21 cells at the depth cap each, and more: Python's integers)
        depth_sum = ((hi.astype(object) << 32) + lo.astype(object)) / 4294967296
        depth_sum = depth_sum.astype(np.float64)
    else:
        depth_sum = (hi.astype(np.float64) * 4294967296.0 + lo.astype(np.float64)) / 4294967296.0
    out["volume"] = depth_sum * (float(dx) * float(dx))
    out["max_depth"] = z[:, :, 5].copy().view(np.float64)
    out["max_speed"] = z[:, :, 6].copy().view(np.float64)
    return out


COMM_ID_BYTES = 128
PEER_TICKET_BYTES = 384


def comm_load(path: str | None = None):
    """Load the collective library for the C++ strip loop (hp_strip_*).  In a torch process the copy torch carries is
    used, so that one RCCL (bound to one HIP runtime) serves the whole process."""
    lib = load_library()
    if path is None:
        try:
            import torch
            cand = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
            path = cand if os.path.exists(cand) else None
        except ImportError:
            path = None
    _check(lib, lib.hp_comm_load(path.encode() if path else None), "hp_comm_load")


def comm_unique_id() -> bytes:
    lib = load_library()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib, lib.hp_comm_unique_id(buf), "hp_comm_unique_id")
    return buf.raw


def device_count() -> int:
    lib = load_library()
    n = C.c_int(0)
    _check(lib, lib.hp_device_count(C.byref(n)), "hp_device_count")
    return n.value


def device_info(device: int = 0) -> dict:
    lib = load_library()
    info = DeviceInfo()
    _check(lib, lib.hp_device_info(device, C.byref(info)), "hp_device_info")
    return dict(name=info.name.decode(), arch=info.arch.decode(), compute_units=info.compute_units,
                clock_mhz=info.clock_mhz, global_mem_bytes=info.global_mem_bytes,
                lds_bytes_per_cu=info.lds_bytes_per_cu, wavefront=info.wavefront, fp64=bool(info.fp64))


class _RecordLog:
    """The host side of a recorder's record log (hp_probes_* / hp_zones_*): the records read back whenever the device buffer was
    full, and which of them a state_restore keeps.  The three callables are the library's: info() -> (samples in the device
    buffer, its capacity, words per record), read(out) fills out[pending, stride] and returns once it has landed, reset() empties
    the device buffer."""

    def __init__(self, dtype, info, read, reset):
        self.dtype, self._info, self._read, self._reset = dtype, info, read, reset
        self.on = False
        self.drained = []                               # records read back when the device buffer was full: [k, stride] arrays
        self.generation = 0                             # counts opened / closed / reset: a checkpoint's count belongs to one
        self.saved_at = None                            # saved()'s (generation, samples so far)

    def opened(self):
        self.on, self.drained = True, []
        self.generation += 1

    def closed(self):
        self.on, self.drained = False, []
        self.generation += 1

    def info(self):
        n, capacity, stride = self._info()
        return dict(samples=sum(len(a) for a in self.drained) + n, pending=n, capacity=capacity, stride=stride)

    def pending(self):
        info = self.info()
        out = np.empty((info["pending"], info["stride"]), self.dtype)
        if info["pending"]:
            self._read(out)
        return out

    def before_sample(self):
        """A full device buffer is read back and emptied (one copy, one sync per `capacity` samples)."""
        info = self.info() if self.on else None         # (not recording: the library's own answer to the sample)
        if info and info["pending"] == info["capacity"]:
            self.drained.append(self.pending())
            self._reset()

    def records(self):
        return np.concatenate(self.drained + [self.pending()], axis=0)

    def reset(self):
        self._reset()
        self.drained = []
        self.generation += 1

    def saved(self):
        self.saved_at = (self.generation, self.info()["samples"]) if self.on else None

    def restored(self):
        """The library's count is the saved one again (0 if the checkpoint is not this generation's): the records read back
        already follow it."""
        if not self.on:
            return
        total = self.saved_at[1] if self.saved_at and self.saved_at[0] == self.generation else 0
        drained = np.concatenate(self.drained, axis=0) if self.drained else None
        keep = max(0, total - self.info()["pending"])
        self.drained = [drained[:keep]] if drained is not None and keep else []


class _DevicePointer:
    """Raw device allocation exposed through __cuda_array_interface__ so torch can wrap it without a copy."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=3,
                                             strides=None)


class Domain:
    """One Cartesian domain (or one row strip of it) resident on one GPU.

    Method names follow the reference's scheme/executor surface for this path:
    ``upload`` = COCLBuffer::queueWriteAll, ``download`` = readDomainAll/queueReadAll,
    ``step_batch`` = the scheduleIteration loop of Threaded_runBatch, ``read_scalars`` = readKeyStatistics,
    ``sync`` = COCLDevice::blockUntilFinished, ``set_target_time`` / ``force_timestep`` = CScheme's.
    """

    def __init__(self, cols, rows, dx=1.0, scheme=SCHEME_GODUNOV, precision="f64", dry_threshold=1e-10,
                 courant=0.5, t_end=1e30, dynamic_dt=True, dt_fixed=0.001, dt_initial=0.001, friction=True,
                 quirks=QUIRKS_REFERENCE, math_mode=MATH_FAST, kernel=KERNEL_AUTO, device=0,
                 global_rows=0, row_offset=0, ghost_rows=0):
        self.lib = load_library()
        self.cols, self.rows = int(cols), int(rows)
        self.precision = precision
        self.real = np.float64 if precision == "f64" else np.float32
        desc = DomainDesc()
        self.lib.hp_domain_desc_default(C.byref(desc))
        desc.device = device
        desc.cols, desc.rows, desc.dx = self.cols, self.rows, dx
        desc.precision = 8 if precision == "f64" else 4
        desc.scheme = scheme
        desc.courant, desc.dry_threshold = courant, dry_threshold
        desc.friction, desc.dynamic_dt = int(friction), int(dynamic_dt)
        desc.dt_fixed, desc.dt_initial, desc.t_end = dt_fixed, dt_initial, t_end
        desc.quirks, desc.math_mode, desc.kernel = quirks, math_mode, kernel
        desc.global_rows, desc.row_offset = global_rows, row_offset
        desc.ghost_rows = ghost_rows
        self.desc = desc
        self.h = C.c_void_p()
        _check(self.lib, self.lib.hp_domain_create(C.byref(desc), C.byref(self.h)), "hp_domain_create")
        self._keepalive = []
        self._bed_host = None
        self._peak_values = []                          # HP_PEAK_* codes the library tracks (peaks_enable's mask)
        self._probes = None                             # (gauges, sections) the library records (probes_enable's lists)
        self._probe_log = self._record_log("hp_probes", np.float64, C.c_double)
        self._zones = None                              # zone_count the library records (zones_enable's)
        self._zone_log = self._record_log("hp_zones", np.uint64, C.c_uint64)

    def _record_log(self, prefix, dtype, ctype):
        """The host side of the recorder `prefix`, on this domain's hp_*_info, hp_*_read + sync and hp_*_reset."""
        dom = weakref.proxy(self)                       # (no cycle: the domain still goes, and frees the device, with its last reference)
        call = lambda name, *args: _check(dom.lib, getattr(dom.lib, prefix + name)(dom.h, *args), prefix + name)

        def info():
            n, cap, stride = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            call("_info", C.byref(n), C.byref(cap), C.byref(stride))
            return n.value, cap.value, stride.value

        def read(out):
            call("_read", 0, len(out), out.ctypes.data_as(C.POINTER(ctype)))
            dom.sync()
        return _RecordLog(dtype, info, read, lambda: call("_reset"))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.hp_domain_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- transfers ----
    def upload(self, state=None, bed=None, manning=None):
        for which, arr, shape in ((ARRAY_BED, bed, (self.rows, self.cols)),
                                  (ARRAY_MANNING, manning, (self.rows, self.cols)),
                                  (ARRAY_STATE, state, (self.rows, self.cols, 4))):
            if arr is None:
                continue
            a = np.ascontiguousarray(arr, dtype=self.real)
            if a.shape != shape:
                raise ValueError(f"array shape {a.shape} != {shape}")
            if which == ARRAY_BED:
                self._bed_host = a.copy()
            self._keepalive.append(a)
            _check(self.lib, self.lib.hp_domain_upload(self.h, which, a.ctypes.data_as(C.c_void_p), a.nbytes),
                   "hp_domain_upload")
        self.sync()
        self._keepalive.clear()

    def download(self, which=ARRAY_STATE, row0=0, nrows=None):
        nrows = self.rows - row0 if nrows is None else nrows
        shape = (nrows, self.cols, 4) if which == ARRAY_STATE else (nrows, self.cols)
        out = np.empty(shape, self.real)
        _check(self.lib, self.lib.hp_domain_download(self.h, which, out.ctypes.data_as(C.c_void_p), row0, nrows),
               "hp_domain_download")
        self.sync()
        return out

    # ---- the output stage on the device (hp_domain_derive / hp_domain_stats) ----
    def derive(self, values, dtype=np.float64, row0=0, nrows=None):
        """Output rasters derived on the device, without a state download: {name: array[nrows, cols]} for the front end's
        value names (frontend.data_value_code: "maxdepth" wins over "depth").  fp64 rasters are bit-identical to
        frontend.derive_output(name, self.download(), bed, dx); dtype=np.float32 gives those values rounded once."""
        from .frontend import data_value_code
        names = [values] if isinstance(values, str) else list(values)
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("dtype must be float64 or float32")
        nrows = self.rows - row0 if nrows is None else nrows
        codes = []
        for name in names:
            code = OUT_CODES.get(data_value_code(name))
            if code is None:
                raise ValueError(f"unknown output {name}")
            if code not in codes:
                codes.append(code)
        arrays = [np.empty((max(0, nrows), self.cols), dtype) for _ in codes]
        if codes:                                       # (also for nrows == 0: the library checks the range first)
            c_values = (C.c_int * len(codes))(*codes)
            c_rasters = (C.c_void_p * len(codes))(*[a.ctypes.data for a in arrays])
            _check(self.lib, self.lib.hp_domain_derive(self.h, c_values, len(codes), dtype.itemsize, c_rasters, row0, nrows),
                   "hp_domain_derive")
            self.sync()
        out, used = {}, set()
        for name in names:
            k = codes.index(OUT_CODES[data_value_code(name)])
            out[name] = arrays[k].copy() if k in used else arrays[k]        # (two names of one value: separate arrays)
            used.add(k)
        return out

    def overview_shape(self, factor, row0=0, nrows=None):
        """(first_block_row, block_rows, block_cols) of Domain.overview's arrays for rows [row0, row0 + nrows): the library's own
        arithmetic (hp_overview_shape; the module's overview_shape restates it)."""
        nrows = self.rows - row0 if nrows is None else nrows
        first, brows, bcols = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _check(self.lib, self.lib.hp_overview_shape(self.h, int(factor), row0, nrows, C.byref(first), C.byref(brows), C.byref(bcols)),
               "hp_overview_shape")
        return first.value, brows.value, bcols.value

    def overview(self, values, aggregates, factor, dtype=np.float64, row0=0, nrows=None):
        """Block-aggregated overview rasters derived on the device, without a state download: one array [block_rows, block_cols]
        per (value, aggregate) pair (overview_pairs), in order.  Blocks of factor x factor cells anchored to the global grid; row 0
        of the arrays is block row overview_shape(...)[0].  fp64 arrays are bit-identical to frontend.overview(frontend.
        derive_output(name, self.download(), bed, dx), factor, aggregate, row_offset); dtype=np.float32 gives those rounded once."""
        pairs = overview_pairs(values, aggregates)
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("dtype must be float64 or float32")
        nrows = self.rows - row0 if nrows is None else nrows
        if not pairs:
            return []
        _, brows, bcols = self.overview_shape(factor, row0, nrows)       # (also checks the factor and the row range)
        arrays = [np.empty((brows, bcols), dtype) for _ in pairs]
        c_values = (C.c_int * len(pairs))(*[v for v, _ in pairs])
        c_aggs = (C.c_int * len(pairs))(*[a for _, a in pairs])
        c_rasters = (C.c_void_p * len(pairs))(*[a.ctypes.data for a in arrays])
        _check(self.lib, self.lib.hp_domain_overview(self.h, c_values, c_aggs, len(pairs), int(factor), dtype.itemsize, c_rasters, row0, nrows),
               "hp_domain_overview")
        self.sync()
        return arrays

    def sparse(self, values, select="depth", above=0.0, dtype=np.float64, row0=0, nrows=None):
        """The values at the selected cells only, compacted on the device (hp_domain_sparse): (row_ptr, col, [one array per value])
        in CSR over rows [row0, row0 + nrows) -- row_ptr uint64 [nrows + 1], col uint32 [selected], entries ascending by (row,
        column).  A cell is selected iff its `select` value v (fp64, before any rounding) satisfies v != -9999 and v > above.
        Bit-identical to frontend.sparse([frontend.derive_output(name, self.download(), bed, dx) ...], derive_output(select, ...),
        above); dtype=np.float32 gives those values rounded once.  One call with room for the previous call's total x 1.25 (the
        first call only counts), a second one if the total has outgrown that."""
        from .frontend import data_value_code
        names = [values] if isinstance(values, str) else list(values)
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("dtype must be float64 or float32")
        codes = [OUT_CODES.get(data_value_code(name)) for name in names]
        select_code = OUT_CODES.get(data_value_code(select))
        if None in codes or select_code is None:
            raise ValueError(f"unknown output {select if select_code is None else names[codes.index(None)]}")
        if len(set(codes)) != len(codes) or not codes:
            raise ValueError("one to nine values, each at most once")
        nrows = self.rows - row0 if nrows is None else nrows
        row_ptr = np.zeros(max(0, nrows) + 1, np.uint64)
        selected = C.c_uint64(0)
        c_values = (C.c_int * len(codes))(*codes)
        capacity = -(-getattr(self, "_sparse_total", 0) * 5 // 4)
        while True:
            col = np.empty(capacity, np.uint32)
            arrays = [np.empty(capacity, dtype) for _ in codes]
            c_rasters = (C.c_void_p * len(codes))(*[a.ctypes.data for a in arrays]) if capacity else None
            _check(self.lib, self.lib.hp_domain_sparse(self.h, select_code, float(above), c_values, len(codes), dtype.itemsize, capacity, C.byref(selected),
                                                       row_ptr.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       col.ctypes.data_as(C.POINTER(C.c_uint32)) if capacity else None, c_rasters, row0, nrows),
                   "hp_domain_sparse")
            if selected.value <= capacity:
                break
            capacity = selected.value                   # (the total has outgrown the guess: once more, with exactly that)
        self.sync()
        self._sparse_total = n = selected.value
        return row_ptr, col[:n], [a[:n] for a in arrays]

    def stats(self, row0=0, nrows=None):
        """cells, cells_wet, volume (m3), max_depth, max_speed and the local flat cell id of each maximum (None where no
        cell qualifies) over rows [row0, row0 + nrows); blocks.  See hp_domain_stats_t for the definitions."""
        nrows = self.rows - row0 if nrows is None else nrows
        s = DomainStats()
        s.struct_size = C.sizeof(DomainStats)
        _check(self.lib, self.lib.hp_domain_stats(self.h, row0, nrows, C.byref(s)), "hp_domain_stats")
        return dict(cells=s.cells, cells_wet=s.cells_wet, volume=s.volume, max_depth=s.max_depth, max_speed=s.max_speed,
                    max_depth_cell=None if s.max_depth_cell == NO_CELL else s.max_depth_cell,
                    max_speed_cell=None if s.max_speed_cell == NO_CELL else s.max_speed_cell)

    # ---- the peak tracker (hp_peaks_*): maxima over the SAMPLES the host takes between batches ----
    @staticmethod
    def _peak_codes(values):
        names = [values] if isinstance(values, str) else list(values)
        codes = []
        for name in names:
            code = name if isinstance(name, int) else PEAK_CODES.get(str(name).lower())
            if code is None or not 0 <= code < PEAK_COUNT:
                raise ValueError(f"unknown peak value {name}")
            codes.append(code)
        return names, codes

    def peaks_enable(self, values, arrival_depth=0.01):
        """Start tracking `values` (names of PEAK_CODES or HP_PEAK_* codes): allocates one fp64 accumulator raster per value
        on the device and resets them; t_previous of the first sample is the device time now."""
        _, codes = self._peak_codes(values)
        desc = PeaksDesc(C.sizeof(PeaksDesc), sum(1 << c for c in set(codes)), float(arrival_depth))
        rc = self.lib.hp_peaks_enable(self.h, C.byref(desc))
        if rc == -3:                                    # HP_ERR_HIP: the allocation failed and the library has switched tracking off
            self._peak_values = []                      # (an argument or state error leaves the tracker as it was)
        _check(self.lib, rc, "hp_peaks_enable")
        self._peak_values = sorted(set(codes))

    def peaks_disable(self):
        _check(self.lib, self.lib.hp_peaks_disable(self.h), "hp_peaks_disable")
        self._peak_values = []

    def peaks_reset(self):
        _check(self.lib, self.lib.hp_peaks_reset(self.h), "hp_peaks_reset")

    def peaks_sample(self):
        """Fold the current state into the accumulators: one launch on the domain's stream, never blocks."""
        _check(self.lib, self.lib.hp_peaks_sample(self.h), "hp_peaks_sample")

    def peaks(self, values=None, dtype=np.float64, row0=0, nrows=None):
        """The peaks so far: {name: array[nrows, cols]} (values=None: every enabled value, by its PEAK_CODES name).  fp64
        arrays are the accumulators, bit-identical to frontend.PeakTracker fed the same samples; dtype=np.float32 gives
        those values rounded once."""
        if values is None:
            if not self._peak_values:
                self.peaks_info()                       # not tracking: the library's own answer (HP_ERR_STATE), not an empty dict
            by_code = {c: n for n, c in PEAK_CODES.items()}
            values = [by_code[c] for c in self._peak_values]
        names, codes = self._peak_codes(values)
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("dtype must be float64 or float32")
        nrows = self.rows - row0 if nrows is None else nrows
        arrays = [np.empty((max(0, nrows), self.cols), dtype) for _ in codes]
        if codes:                                       # (also for nrows == 0: the library checks the range first)
            c_values = (C.c_int * len(codes))(*codes)
            c_rasters = (C.c_void_p * len(codes))(*[a.ctypes.data for a in arrays])
            _check(self.lib, self.lib.hp_peaks_read(self.h, c_values, len(codes), dtype.itemsize, c_rasters, row0, nrows),
                   "hp_peaks_read")
            self.sync()
        return dict(zip(names, arrays))

    def peaks_info(self):
        """dict(samples, t_first, t_last): samples taken since enable / reset and the model times of the first and the
        last of them; blocks."""
        n, t0, t1 = C.c_uint64(0), C.c_double(0.0), C.c_double(0.0)
        _check(self.lib, self.lib.hp_peaks_info(self.h, C.byref(n), C.byref(t0), C.byref(t1)), "hp_peaks_info")
        return dict(samples=n.value, t_first=t0.value, t_last=t1.value)

    # ---- the probe recorder (hp_probes_*): gauge and cross-section time series, one record per SAMPLE the host takes ----
    def probes_enable(self, gauges=(), sections=(), capacity=4096):
        """Start recording: `gauges` are (x, y) cell indices, `sections` (cells, wx, wy) triples -- cells as (x, y) pairs, one
        weight pair in {-1, 0, 1} per cell -- or what frontend.rasterise_section returns.  `capacity` is the number of samples
        the device buffer holds; probes_sample() drains a full buffer by itself, so it only sets how often that happens."""
        def flat(cells):
            c = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
            if c.size and (c.min() < 0 or (c[:, 0] >= self.cols).any() or (c[:, 1] >= self.rows).any()):
                raise ValueError("a probe cell lies outside the domain")
            return c[:, 1] * self.cols + c[:, 0]
        self.probes_enable_cells(flat(gauges), [(flat(s[0]), s[1], s[2]) for s in sections], capacity)

    def probes_enable_cells(self, gauge_cells, sections=(), capacity=4096):
        """probes_enable with flat cell ids y * cols + x of the local array (what hp_probes_desc_t takes; not range-checked
        here: the library does that)."""
        g = np.ascontiguousarray(gauge_cells, dtype=np.uint64).reshape(-1)
        offsets = np.zeros(len(sections) + 1, np.uint64)
        offsets[1:] = np.cumsum([len(np.reshape(s[0], -1)) for s in sections], dtype=np.uint64)
        join = lambda k, dtype: np.ascontiguousarray(np.concatenate([np.asarray(s[k]).reshape(-1) for s in sections]), dtype=dtype) \
            if len(sections) else np.zeros(0, dtype)
        for s in sections:
            if not len(np.reshape(s[0], -1)) == len(np.reshape(s[1], -1)) == len(np.reshape(s[2], -1)):
                raise ValueError("a section needs one weight pair per cell")
        cells, wx, wy = join(0, np.uint64), join(1, np.int8), join(2, np.int8)
        desc = ProbesDesc(C.sizeof(ProbesDesc), int(capacity), g.size, g.ctypes.data_as(C.POINTER(C.c_uint64)), len(sections),
                          offsets.ctypes.data_as(C.POINTER(C.c_uint64)), cells.ctypes.data_as(C.POINTER(C.c_uint64)),
                          wx.ctypes.data_as(C.POINTER(C.c_int8)), wy.ctypes.data_as(C.POINTER(C.c_int8)))
        rc = self.lib.hp_probes_enable(self.h, C.byref(desc))
        if rc == -3:                                    # HP_ERR_HIP: the allocation failed and the library has switched recording off
            self._probes = None                         # (an argument or state error leaves the recorder as it was)
            self._probe_log.closed()
        _check(self.lib, rc, "hp_probes_enable")
        self._probes = (int(g.size), len(sections))
        self._probe_log.opened()

    def probes_disable(self):
        _check(self.lib, self.lib.hp_probes_disable(self.h), "hp_probes_disable")
        self._probes = None
        self._probe_log.closed()

    def probes_info(self):
        """dict(samples, pending, capacity, stride): samples taken since probes_enable, how many of them are still in the device
        buffer, that buffer's capacity and the record length in fp64 words; host-side counters, does not block."""
        return self._probe_log.info()

    def probes_sample(self):
        """One record of the current state: one launch on the domain's stream.  Does not block -- except when the device buffer
        is full: then its records are read back first (one copy, one sync per `capacity` samples)."""
        self._probe_log.before_sample()
        _check(self.lib, self.lib.hp_probes_sample(self.h), "hp_probes_sample")

    def probes(self):
        """Every sample since probes_enable, in order: {"t": [n], "gauges": [n, G, 4] (z, depth, qx, qy), "sections": [n, S]
        (discharge, m3/s)}, bit-identical to frontend.ProbeRecorder fed the same samples; blocks."""
        return split_probe_records(self._probe_log.records(), *self._probes)

    # ---- the zone recorder (hp_zones_*): per-zone counts, volume, largest depth and speed, one record per SAMPLE the host takes ----
    def zones_enable(self, ids, zone_count=None, flood_depth=0.1, capacity=4096):
        """Start recording: `ids` is the [rows, cols] raster of zone ids of the local array (row 0 = south; 0 = in no zone),
        `zone_count` the number of zones (default: the largest id), `flood_depth` the "flooded" threshold in metres.  `capacity`
        is the number of samples the device buffer holds; zones_sample() drains a full buffer by itself."""
        a = np.asarray(ids)
        if a.shape != (self.rows, self.cols):
            raise ValueError(f"the zone raster must be [{self.rows}, {self.cols}]")
        if a.dtype.kind not in "iu":
            if not np.array_equal(a, np.round(a)):
                raise ValueError("zone ids must be integers")
        if a.size and (a.min() < 0 or a.max() > 65535):
            raise ValueError("zone ids must lie in 0..65535")
        ids16 = np.ascontiguousarray(a, dtype=np.uint16)
        count = int(zone_count) if zone_count is not None else max(1, int(ids16.max()) if ids16.size else 1)
        if not 0 <= count < 2 ** 32:
            raise ValueError("zone_count out of range")
        self.zones_enable_raw(ids16, count, flood_depth, capacity)

    def zones_enable_raw(self, ids16, zone_count, flood_depth=0.1, capacity=4096):
        """zones_enable with what hp_zones_desc_t takes (a contiguous uint16 array of cols * rows ids; not checked here: the
        library does that)."""
        ids16 = np.ascontiguousarray(ids16, dtype=np.uint16)
        desc = ZonesDesc(C.sizeof(ZonesDesc), int(capacity), int(zone_count), 0, ids16.ctypes.data_as(C.POINTER(C.c_uint16)), float(flood_depth))
        rc = self.lib.hp_zones_enable(self.h, C.byref(desc))
        if rc == -3:                                    # HP_ERR_HIP: the allocation failed and the library has switched recording off
            self._zones = None
            self._zone_log.closed()
        _check(self.lib, rc, "hp_zones_enable")
        self._zones = int(zone_count)
        self._zone_log.opened()

    def zones_disable(self):
        _check(self.lib, self.lib.hp_zones_disable(self.h), "hp_zones_disable")
        self._zones = None
        self._zone_log.closed()

    def zones_reset(self):
        """Forget every sample taken so far (those read back already too)."""
        self._zone_log.reset()

    def zones_info(self):
        """dict(samples, pending, capacity, stride): samples taken since zones_enable / zones_reset, how many of them are still in
        the device buffer, that buffer's capacity and the record length in 64-bit words; host-side counters, does not block."""
        return self._zone_log.info()

    def zones_sample(self):
        """One record of the current state: one fill and one launch on the domain's stream.  Does not block -- except when the
        device buffer is full: then its records are read back first (one copy, one sync per `capacity` samples)."""
        self._zone_log.before_sample()
        _check(self.lib, self.lib.hp_zones_sample(self.h), "hp_zones_sample")

    def zone_records(self):
        """Every record since zones_enable, in order: uint64 [n, 1 + 7 Z] (hp_zones_read's layout); blocks."""
        return self._zone_log.records()

    def zones(self):
        """Every sample since zones_enable, in order (split_zone_records' dictionary), equal in every word to frontend.ZoneRecorder
        fed the same samples; blocks."""
        return split_zone_records(self.zone_records(), self._zones, self.desc.dx)

    def upload_rows(self, rows_state, row0):
        a = np.ascontiguousarray(rows_state, dtype=self.real)
        _check(self.lib, self.lib.hp_domain_upload_rows(self.h, a.ctypes.data_as(C.c_void_p), row0, a.shape[0]),
               "hp_domain_upload_rows")
        self.sync()

    def state_save(self):
        """Device-side checkpoint of cell states + time-control block (saveCurrentState without the PCIe trip)."""
        _check(self.lib, self.lib.hp_state_save(self.h), "hp_state_save")
        self._probe_log.saved()
        self._zone_log.saved()

    def state_restore(self):
        _check(self.lib, self.lib.hp_state_restore(self.h), "hp_state_restore")
        self._probe_log.restored()
        self._zone_log.restored()

    # ---- the moving bed (hp_bed_*): the bed at listed cells follows a schedule, applied between batches on the device ----
    def bed_shape_add(self, cells, target, series):
        """One shape: `cells` are flat ids y * cols + x of the GLOBAL grid or (x, y) pairs, `target` one elevation per cell (or one
        for all of them), `series` [n, 2] rows of (time, fraction).  The shape's base is the bed as it is now."""
        c = np.asarray(cells)
        if c.ndim == 2 and c.shape[1] == 2:
            c = c.astype(np.int64)
            if c.size and (c.min() < 0 or (c[:, 0] >= self.cols).any()):
                raise ValueError("a bed shape's cell lies outside the grid")
            c = c[:, 1] * self.cols + c[:, 0]
        c = np.ascontiguousarray(c, dtype=np.uint64).reshape(-1)
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(target, dtype=np.float64), c.shape))
        s = np.ascontiguousarray(series, dtype=np.float64).reshape(-1, 2)
        desc = BedShapeDesc(C.sizeof(BedShapeDesc), len(s), c.size, c.ctypes.data_as(C.POINTER(C.c_uint64)),
                            t.ctypes.data_as(C.POINTER(C.c_double)), s.ctypes.data_as(C.POINTER(C.c_double)))
        _check(self.lib, self.lib.hp_bed_shape_add(self.h, C.byref(desc)), "hp_bed_shape_add")

    def bed_shapes_clear(self):
        _check(self.lib, self.lib.hp_bed_shapes_clear(self.h), "hp_bed_shapes_clear")

    def bed_apply(self):
        """Move the bed of the listed cells to where the shapes' series put it at the device's own time: one launch and one
        device copy of the state on the domain's stream, equal in every bit to download, frontend.BedShapes.apply and upload of
        bed and state.  Does not block."""
        _check(self.lib, self.lib.hp_bed_apply(self.h), "hp_bed_apply")

    def bed_info(self):
        """dict(shapes, cells_local, applies, changed_last, changed_total, t_last); blocks."""
        info = BedInfo(C.sizeof(BedInfo))
        _check(self.lib, self.lib.hp_bed_info(self.h, C.byref(info)), "hp_bed_info")
        return {k: getattr(info, k) for k, _ in BedInfo._fields_ if k != "struct_size"}

    # ---- boundaries ----
    def add_uniform(self, definition, series, interval, length):
        s = np.ascontiguousarray(series, dtype=self.real)
        assert s.ndim == 2 and s.shape[1] == 2
        _check(self.lib, self.lib.hp_boundary_add_uniform(self.h, definition, s.ctypes.data_as(C.c_void_p),
                                                          s.shape[0], interval, length), "hp_boundary_add_uniform")

    def add_gridded(self, definition, grids, resolution, off_x, off_y, interval):
        g = np.ascontiguousarray(grids, dtype=self.real)
        assert g.ndim == 3
        _check(self.lib, self.lib.hp_boundary_add_gridded(self.h, definition, g.ctypes.data_as(C.c_void_p), g.shape[0],
                                                          g.shape[1], g.shape[2], resolution, off_x, off_y, interval),
               "hp_boundary_add_gridded")

    def add_cell(self, depth_def, discharge_def, cells, series, interval, length):
        rel = np.ascontiguousarray(cells, dtype=np.uint64)
        ser = np.ascontiguousarray(series, dtype=self.real)
        assert ser.ndim == 2 and ser.shape[1] == 4
        _check(self.lib, self.lib.hp_boundary_add_cell(self.h, depth_def, discharge_def, rel.ctypes.data_as(C.c_void_p),
                                                       rel.size, ser.ctypes.data_as(C.c_void_p), ser.shape[0], interval,
                                                       length), "hp_boundary_add_cell")

    def add_links(self, links):
        """One link group (hp_boundary_add_links): water passes between two distant cells as a function of their own levels -- weirs,
        orifices / culverts, pumps.  `links`: see pack_links; ids are GLOBAL.  Applied per iteration at its place in the order the
        boundaries were added; frontend.Links is the same arithmetic on the host, bit for bit."""
        a = pack_links(links, self.cols)
        _check(self.lib, self.lib.hp_boundary_add_links(self.h, a.ctypes.data_as(C.c_void_p), a.size), "hp_boundary_add_links")

    def links_info(self):
        """dict(links, groups): host counters."""
        n, g = C.c_uint64(0), C.c_uint64(0)
        _check(self.lib, self.lib.hp_links_info(self.h, C.byref(n), C.byref(g)), "hp_links_info")
        return dict(links=n.value, groups=g.value)

    def links_read(self, first=0, count=None):
        """The links' records as an array of LINK_RECORD_DTYPE (q_last, volume, active), in the order added; blocks."""
        count = self.links_info()["links"] - first if count is None else count
        out = np.zeros(count, LINK_RECORD_DTYPE)
        _check(self.lib, self.lib.hp_links_read(self.h, first, count, out.ctypes.data_as(C.c_void_p)), "hp_links_read")
        self.sync()
        return out

    def add_open(self, segments):
        """The open boundary (hp_boundary_add_open): every ring cell of the segments takes the depth and the outward momentum of its
        inward neighbour once per iteration, at its place in the order the boundaries were added, and records the discharge that leaves
        through its face.  `segments`: see pack_open_segments -- dict(edge="east", first=.., last=..), or just "east" for the whole
        edge; indices are GLOBAL.  frontend.Open is the same arithmetic on the host, bit for bit."""
        a = pack_open_segments(segments, self.cols, int(self.desc.global_rows) or self.rows)
        _check(self.lib, self.lib.hp_boundary_add_open(self.h, a.ctypes.data_as(C.c_void_p), a.size), "hp_boundary_add_open")

    def open_info(self):
        """dict(segments, cells): host counters."""
        n, c = C.c_uint32(0), C.c_uint64(0)
        _check(self.lib, self.lib.hp_open_info(self.h, C.byref(n), C.byref(c)), "hp_open_info")
        return dict(segments=n.value, cells=c.value)

    def open_read(self, first=0, count=None):
        """The open cells' records as an array of OPEN_RECORD_DTYPE (q_last, volume, active): by segment in the order added, by
        ascending index inside a segment; blocks."""
        count = self.open_info()["cells"] - first if count is None else count
        out = np.zeros(count, OPEN_RECORD_DTYPE)
        _check(self.lib, self.lib.hp_open_read(self.h, first, count, out.ctypes.data_as(C.c_void_p)), "hp_open_read")
        self.sync()
        return out

    def add_infiltration(self, soil, classes, initial=None):
        """The infiltration (hp_boundary_add_infiltration): Green-Ampt by soil class, applied per iteration at its place in the order
        the boundaries were added.  `soil`: [rows, cols] class ids of the LOCAL array (row 0 = south; 0 = impervious), `classes`: see
        pack_soil_classes (class k is entry k - 1), `initial`: [rows, cols] cumulative infiltration in m for a hot start, or None for
        zeros.  frontend.Infiltration is the same arithmetic on the host, bit for bit."""
        ids = soil_ids(soil)
        if ids.shape != (self.rows, self.cols):
            raise ValueError(f"the soil raster must be [{self.rows}, {self.cols}]")
        cls = pack_soil_classes(classes)
        f0 = None
        if initial is not None:
            f0 = np.ascontiguousarray(initial, dtype=np.float64)
            if f0.shape != (self.rows, self.cols):
                raise ValueError(f"the initial infiltration must be [{self.rows}, {self.cols}]")
        desc = InfiltrationDesc(C.sizeof(InfiltrationDesc), len(cls), cls.ctypes.data if len(cls) else None, ids.ctypes.data,
                                None if f0 is None else f0.ctypes.data)
        _check(self.lib, self.lib.hp_boundary_add_infiltration(self.h, C.byref(desc)), "hp_boundary_add_infiltration")

    def infiltration_info(self):
        """dict(classes, pervious_cells): host counters (both 0 without an infiltration)."""
        n, c = C.c_uint32(0), C.c_uint64(0)
        _check(self.lib, self.lib.hp_infiltration_info(self.h, C.byref(n), C.byref(c)), "hp_infiltration_info")
        return dict(classes=n.value, pervious_cells=c.value)

    def infiltration_read(self, row0=0, nrows=None):
        """The cumulative infiltrated depth F in m, fp64 [nrows, cols] (default: every row of the local array); blocks."""
        nrows = self.rows - row0 if nrows is None else nrows
        out = np.zeros((max(0, nrows), self.cols), np.float64)
        _check(self.lib, self.lib.hp_infiltration_read(self.h, out.ctypes.data, row0, nrows), "hp_infiltration_read")
        self.sync()
        return out

    def tracer_enable(self, initial=None):
        """The passive tracer (hp_tracer_enable): a solute mass per unit area M, fp64, moved once per iteration by the mass fluxes of
        the flux kernel's exact face solve, upwinded.  `initial`: [rows, cols] M0 in units * m (row 0 = south), or None for zeros.
        frontend.Tracer is the same arithmetic on the host, bit for bit."""
        m0 = None
        if initial is not None:
            m0 = np.ascontiguousarray(initial, dtype=np.float64)
            if m0.shape != (self.rows, self.cols):
                raise ValueError(f"the initial tracer must be [{self.rows}, {self.cols}]")
        desc = TracerDesc(C.sizeof(TracerDesc), 0, None if m0 is None else m0.ctypes.data)
        _check(self.lib, self.lib.hp_tracer_enable(self.h, C.byref(desc)), "hp_tracer_enable")

    def tracer_enable_set(self, initial=None, decay=None, species=None):
        """A tracer set (hp_tracer_enable_set): K species moved by one launch per iteration, the face fluxes formed once, each with a
        first-order decay rate.  `initial`: [K, rows, cols] M0 or None for zeros; `decay`: K rates in 1/s or None for zeros; `species`:
        K, needed only when neither says it.  frontend.TracerSet is the same arithmetic on the host, bit for bit."""
        m0 = lam = None
        if initial is not None:
            m0 = np.ascontiguousarray(initial, dtype=np.float64)
            if m0.ndim != 3 or m0.shape[1:] != (self.rows, self.cols):
                raise ValueError(f"the initial tracers must be [species, {self.rows}, {self.cols}]")
        if decay is not None:
            lam = np.ascontiguousarray(decay, dtype=np.float64).reshape(-1)
        said = ([] if species is None else [int(species)]) + ([] if m0 is None else [m0.shape[0]]) + ([] if lam is None else [lam.size])
        if not said or len(set(said)) != 1:
            raise ValueError("species, initial and decay must name one number of species")
        desc = TracerSetDesc(C.sizeof(TracerSetDesc), said[0], None if lam is None or not lam.size else lam.ctypes.data,
                             None if m0 is None or not m0.size else m0.ctypes.data)
        _check(self.lib, self.lib.hp_tracer_enable_set(self.h, C.byref(desc)), "hp_tracer_enable_set")

    def tracer_disable(self):
        _check(self.lib, self.lib.hp_tracer_disable(self.h), "hp_tracer_disable")

    def tracer_add_source(self, cells, series, species=0):
        """One source (hp_tracer_add_source; hp_tracer_add_source_to for a `species` other than 0): `cells` flat ids (y * cols + x) or
        (x, y) pairs, `series` [(time, mass rate)]: every listed cell receives the rate, interpolated by the bed shapes' rule."""
        c = np.asarray(cells)
        if c.ndim == 2:
            c = c[:, 1].astype(np.uint64) * np.uint64(self.cols) + c[:, 0].astype(np.uint64)
        c = np.ascontiguousarray(c, dtype=np.uint64).reshape(-1)
        s = np.ascontiguousarray(series, dtype=np.float64).reshape(-1, 2)
        if species:
            _check(self.lib, self.lib.hp_tracer_add_source_to(self.h, species, c.ctypes.data if c.size else None, c.size, s.ctypes.data if s.size else None, len(s)),
                   "hp_tracer_add_source_to")
            return
        _check(self.lib, self.lib.hp_tracer_add_source(self.h, c.ctypes.data if c.size else None, c.size, s.ctypes.data if s.size else None, len(s)),
               "hp_tracer_add_source")

    def tracer_sources_clear(self):
        _check(self.lib, self.lib.hp_tracer_sources_clear(self.h), "hp_tracer_sources_clear")

    def tracer_read(self, row0=0, nrows=None, species=0):
        """The current M in units * m, fp64 [nrows, cols] (default: every row of the local array), of `species` of a set; blocks."""
        nrows = self.rows - row0 if nrows is None else nrows
        out = np.zeros((max(0, nrows), self.cols), np.float64)
        if species:
            _check(self.lib, self.lib.hp_tracer_read_species(self.h, species, out.ctypes.data, row0, nrows), "hp_tracer_read_species")
        else:
            _check(self.lib, self.lib.hp_tracer_read(self.h, out.ctypes.data, row0, nrows), "hp_tracer_read")
        self.sync()
        return out

    def tracer_write(self, raster, row0=0, species=0):
        """Replace rows row0 .. of the current M (of `species` of a set) by `raster` [nrows, cols]."""
        m = np.ascontiguousarray(raster, dtype=np.float64)
        if m.ndim != 2 or m.shape[1] != self.cols:
            raise ValueError(f"the raster must be [nrows, {self.cols}]")
        if species:
            _check(self.lib, self.lib.hp_tracer_write_species(self.h, species, m.ctypes.data, row0, m.shape[0]), "hp_tracer_write_species")
        else:
            _check(self.lib, self.lib.hp_tracer_write(self.h, m.ctypes.data, row0, m.shape[0]), "hp_tracer_write")

    def tracer_info(self):
        """dict(iterations, sources, source_cells): host counters (all 0 without a tracer)."""
        n, s, c = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        _check(self.lib, self.lib.hp_tracer_info(self.h, C.byref(n), C.byref(s), C.byref(c)), "hp_tracer_info")
        return dict(iterations=n.value, sources=s.value, source_cells=c.value)

    def tracer_set_info(self):
        """dict(species, decay): K (0 without a tracer, 1 for a single one) and the K decay rates."""
        k, lam = C.c_uint32(0), (C.c_double * TRACER_MAX_SPECIES)()
        _check(self.lib, self.lib.hp_tracer_set_info(self.h, C.byref(k), lam), "hp_tracer_set_info")
        return dict(species=k.value, decay=[float(v) for v in lam[:k.value]])

    def tracer_set_exchange(self, species, settling=0.0, tau_deposit=float("inf"), tau_erode=float("inf"), erodibility=0.0, deposit=None):
        """Let `species` of a tracer set exchange mass with its deposit D on the ground (hp_tracer_set_exchange): it settles at
        `settling` m/s where the bed shear stress is below `tau_deposit` N/m2 (Krone) and is eroded at `erodibility` units/(m2 s)
        where it exceeds `tau_erode` (Partheniades).  `deposit`: D0 [rows, cols], or None: zeros on the domain's first call, D as it
        is on a later one.  frontend.Tracer(exchange=...) is the same arithmetic on the host, bit for bit."""
        d0 = None
        if deposit is not None:
            d0 = np.ascontiguousarray(deposit, dtype=np.float64)
            if d0.shape != (self.rows, self.cols):
                raise ValueError(f"the initial deposit must be [{self.rows}, {self.cols}]")
        desc = TracerExchangeDesc(C.sizeof(TracerExchangeDesc), species, settling, tau_deposit, tau_erode, erodibility, None if d0 is None else d0.ctypes.data)
        _check(self.lib, self.lib.hp_tracer_set_exchange(self.h, C.byref(desc)), "hp_tracer_set_exchange")

    def tracer_deposit_read(self, species=0, row0=0, nrows=None):
        """The deposit D of `species` in units * m, fp64 [nrows, cols] (default: every row of the local array); blocks."""
        nrows = self.rows - row0 if nrows is None else nrows
        out = np.zeros((max(0, nrows), self.cols), np.float64)
        _check(self.lib, self.lib.hp_tracer_deposit_read(self.h, species, out.ctypes.data, row0, nrows), "hp_tracer_deposit_read")
        self.sync()
        return out

    def tracer_deposit_write(self, raster, species=0, row0=0):
        """Replace rows row0 .. of the deposit D of `species` by `raster` [nrows, cols]."""
        m = np.ascontiguousarray(raster, dtype=np.float64)
        if m.ndim != 2 or m.shape[1] != self.cols:
            raise ValueError(f"the raster must be [nrows, {self.cols}]")
        _check(self.lib, self.lib.hp_tracer_deposit_write(self.h, species, m.ctypes.data, row0, m.shape[0]), "hp_tracer_deposit_write")

    def tracer_exchange_info(self):
        """dict(exchanging, species): how many species exchange with a deposit, and per species of the set what was set
        (settling, tau_deposit, tau_erode, erodibility; never set: 0, inf, inf, 0)."""
        n, out = C.c_uint32(0), (TracerExchangeDesc * TRACER_MAX_SPECIES)()
        _check(self.lib, self.lib.hp_tracer_exchange_info(self.h, C.byref(n), out), "hp_tracer_exchange_info")
        k = self.tracer_set_info()["species"]
        return dict(exchanging=n.value, species=[dict(settling=q.settling, tau_deposit=q.tau_deposit, tau_erode=q.tau_erode, erodibility=q.erodibility)
                                                  for q in out[:k]])

    def clear_boundaries(self):
        _check(self.lib, self.lib.hp_boundary_clear(self.h), "hp_boundary_clear")

    def boundaries_fused(self):
        """True when rain / loss ride in the flux kernel's store epilogue instead of a pass of their own."""
        f = C.c_int(0)
        _check(self.lib, self.lib.hp_boundaries_fused(self.h, C.byref(f)), "hp_boundaries_fused")
        return bool(f.value)

    # ---- time control / stepping ----
    def set_target_time(self, t):
        _check(self.lib, self.lib.hp_set_target_time(self.h, t), "hp_set_target_time")

    set_target = set_target_time

    def set_time(self, t):
        _check(self.lib, self.lib.hp_set_time(self.h, t), "hp_set_time")

    def force_timestep(self, dt):
        _check(self.lib, self.lib.hp_force_timestep(self.h, dt), "hp_force_timestep")

    def reset_counters(self):
        _check(self.lib, self.lib.hp_reset_counters(self.h), "hp_reset_counters")

    def update_timestep(self):
        _check(self.lib, self.lib.hp_update_timestep(self.h), "hp_update_timestep")

    def step_batch(self, n):
        _check(self.lib, self.lib.hp_step_batch(self.h, int(n)), "hp_step_batch")

    def step_begin(self):
        _check(self.lib, self.lib.hp_step_begin(self.h), "hp_step_begin")

    def step_end(self):
        _check(self.lib, self.lib.hp_step_end(self.h), "hp_step_end")

    def step_needs_reduction(self):
        f = C.c_int(0)
        _check(self.lib, self.lib.hp_step_needs_reduction(self.h, C.byref(f)), "hp_step_needs_reduction")
        return bool(f.value)

    # ---- the strip loop in C++ over RCCL (hp_strip_*) ----
    def strip_comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == COMM_ID_BYTES
        _check(self.lib, self.lib.hp_strip_comm_init(self.h, unique_id, rank, world), "hp_strip_comm_init")

    def strip_step_batch(self, n):
        _check(self.lib, self.lib.hp_strip_step_batch(self.h, int(n)), "hp_strip_step_batch")

    def strip_update_timestep(self):
        _check(self.lib, self.lib.hp_strip_update_timestep(self.h), "hp_strip_update_timestep")

    def strip_info(self):
        info = StripInfo()
        _check(self.lib, self.lib.hp_strip_info(self.h, C.byref(info)), "hp_strip_info")
        return dict(library=info.library.decode(errors="replace"), comm_ranks=info.comm_ranks, comm_rank=info.comm_rank,
                    halo_overlap=bool(info.halo_overlap), ghost_rows=info.ghost_rows, peer_max=bool(info.peer_max),
                    peer_halo=bool(info.peer_halo))

    # ---- the maximum over the strips through peer-written mailboxes (hp_strip_peer_*) ----
    def strip_peer_ticket(self) -> bytes:
        buf = C.create_string_buffer(PEER_TICKET_BYTES)
        _check(self.lib, self.lib.hp_strip_peer_ticket(self.h, buf), "hp_strip_peer_ticket")
        return buf.raw

    def strip_peer_connect(self, tickets, rank) -> int:
        """`tickets`: every rank's ticket, in rank order.  Collective.  0: everything stays with the collective library,
        1: the maximum over the strips goes through the mailboxes, 2: and the ghost rows are written by the strips into
        each other's buffers."""
        blob = b"".join(tickets)
        assert len(blob) == PEER_TICKET_BYTES * len(tickets)
        active = C.c_int(0)
        _check(self.lib, self.lib.hp_strip_peer_connect(self.h, blob, len(tickets), int(rank), C.byref(active)), "hp_strip_peer_connect")
        return int(active.value)

    def strip_peer_round(self, value: float) -> float:
        out = C.c_double(0.0)
        _check(self.lib, self.lib.hp_strip_peer_round(self.h, float(value), C.byref(out)), "hp_strip_peer_round")
        return out.value

    def strip_peer_disconnect(self):
        _check(self.lib, self.lib.hp_strip_peer_disconnect(self.h), "hp_strip_peer_disconnect")

    def strip_comm_destroy(self):
        _check(self.lib, self.lib.hp_strip_comm_destroy(self.h), "hp_strip_comm_destroy")

    def run(self, n):
        """Run n iterations and return the timestep USED by each (one blocking read per iteration: tests only)."""
        trace = np.zeros(n, self.real)
        for i in range(n):
            trace[i] = self.read_scalars()["timestep"]
            self.step_batch(1)
        return trace

    def read_scalars(self):
        out = ScalarsOut()
        _check(self.lib, self.lib.hp_read_scalars(self.h, C.byref(out)), "hp_read_scalars")
        return {k: getattr(out, k) for k, _ in ScalarsOut._fields_}

    def sync(self):
        _check(self.lib, self.lib.hp_sync(self.h), "hp_sync")

    def is_busy(self):
        b = C.c_int(0)
        _check(self.lib, self.lib.hp_is_busy(self.h, C.byref(b)), "hp_is_busy")
        return bool(b.value)

    # ---- raw device access for the strip exchange ----
    def device_ptr(self, which):
        p = C.c_void_p()
        _check(self.lib, self.lib.hp_device_ptr(self.h, which, C.byref(p)), "hp_device_ptr")
        return p.value

    def stream_ptr(self):
        p = C.c_void_p()
        _check(self.lib, self.lib.hp_stream(self.h, C.byref(p)), "hp_stream")
        return p.value or 0

    def halo_stream_ptr(self):
        p = C.c_void_p()
        _check(self.lib, self.lib.hp_stream_halo(self.h, C.byref(p)), "hp_stream_halo")
        return p.value or 0

    def set_halo_overlap(self, on=True):
        _check(self.lib, self.lib.hp_set_halo_overlap(self.h, int(bool(on))), "hp_set_halo_overlap")

    def device_array(self, which):
        """Zero-copy view (``__cuda_array_interface__``) of a device array, for torch.as_tensor(...)."""
        typestr = "<f8" if self.precision == "f64" else "<f4"
        if which in (PTR_STATE_NEXT_SRC, PTR_STATE_OTHER):
            shape = (self.rows, self.cols, 4)
        elif which in (PTR_BED, PTR_MANNING):
            shape = (self.rows, self.cols)
        elif which == PTR_CFL_MAX:
            shape = (1,)
        else:
            raise ValueError(which)
        return _DevicePointer(self.device_ptr(which), shape, typestr)

    # ---- measurement ----
    def timer_start(self):
        _check(self.lib, self.lib.hp_timer_start(self.h), "hp_timer_start")

    def timer_stop(self):
        ms = C.c_float(0)
        _check(self.lib, self.lib.hp_timer_stop(self.h, C.byref(ms)), "hp_timer_stop")
        return ms.value

    def kernel_timing(self, stride):
        _check(self.lib, self.lib.hp_kernel_timing(self.h, stride), "hp_kernel_timing")

    def kernel_timing_read(self):
        avg, n = C.c_double(0), C.c_uint32(0)
        _check(self.lib, self.lib.hp_kernel_timing_read(self.h, C.byref(avg), C.byref(n)), "hp_kernel_timing_read")
        return avg.value, n.value

    def launch_counts(self):
        """(whole-domain flux launches queued so far, how many carried their own tail block); None with a library that
        predates the call (round-4 builds loaded through HIPIMS_MI_LIB for A/B runs)."""
        if not hasattr(self.lib, "hp_launch_counts"):
            return None
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(self.lib, self.lib.hp_launch_counts(self.h, C.byref(a), C.byref(b)), "hp_launch_counts")
        return a.value, b.value

    def pair_stats(self):
        """Diagnostics of the iteration pairs (hp_pair_stats): dict(pairs, cold_starts, stamped_last, stamped_ever); blocks."""
        if not hasattr(self.lib, "hp_pair_stats"):
            return None
        out = (C.c_uint64 * 12)()
        self.lib.hp_pair_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        _check(self.lib, self.lib.hp_pair_stats(self.h, out), "hp_pair_stats")
        return dict(pairs=out[0], cold_starts=out[1], stamped_last=out[2], stamped_ever=out[3], tune_samples=out[4],
                    tune_switches=out[5], prefers_pairs=bool(out[6]), pair_over_single=out[7] / 1000.0, stale_used=out[8],
                    skipped_rows=out[9], still_rows=out[10], reordered_tiles=out[11])

    def pair_wall_stats(self):
        """(window rows next to the edge ring that the last pair launch skipped, such rows it recorded as still): hp_pair_wall_stats."""
        if not hasattr(self.lib, "hp_pair_wall_stats"):      # (absent from older builds loaded through HIPIMS_MI_LIB for A/B runs)
            return None
        out = (C.c_uint64 * 2)()
        self.lib.hp_pair_wall_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        _check(self.lib, self.lib.hp_pair_wall_stats(self.h, out), "hp_pair_wall_stats")
        return out[0], out[1]

    def kernel_timing_overhead(self):
        """Cost of an empty event pair (ms) that kernel_timing_read() has taken off every sample (0.0 with a library that
        predates the call)."""
        if not hasattr(self.lib, "hp_kernel_timing_overhead"):
            return 0.0
        ms = C.c_double(0)
        _check(self.lib, self.lib.hp_kernel_timing_overhead(self.h, C.byref(ms)), "hp_kernel_timing_overhead")
        return ms.value

    # ---- output derivation (src/Datasets/CRasterDataset.cpp:214-251) ----
    def depth_velocity(self, state=None, bed=None):
        state = self.download() if state is None else state
        bed = self._bed_host if bed is None else bed
        depth = np.maximum(0.0, state[..., 0].astype(np.float64) - bed.astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(depth > 1e-8, state[..., 2] / depth, 0.0)
            v = np.where(depth > 1e-8, state[..., 3] / depth, 0.0)
        return depth, u, v
