"""The output stage's interface (hp_domain_derive / hp_domain_stats), without a GPU: the header declares the two calls and
the value enum, the binding's constants and struct are the header's, argument errors are error codes before any device is
touched, the strip runner's combination of per-rank statistics is exact, and a Model over an engine without `derive`
(the oracle) still takes the host path and produces the same outputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hipims_mi as hp
import oracle
from conftest import ROOT
from hipims_mi import frontend, strips
from model_dir import make_newcastle

HEADER = open(os.path.join(ROOT, "include", "hipims_mi.h")).read()


def test_header_declares_the_calls_and_the_binding_matches():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bint\s+hp_domain_derive\s*\(", code) and re.search(r"\bint\s+hp_domain_stats\s*\(", code)
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(HP_OUT_[A-Z_]+)\s*=\s*(\d+)", code))
    want = {"HP_OUT_DEPTH": hp.OUT_DEPTH, "HP_OUT_MAXDEPTH": hp.OUT_MAXDEPTH, "HP_OUT_FSL": hp.OUT_FSL, "HP_OUT_MAXFSL": hp.OUT_MAXFSL,
            "HP_OUT_DISCHARGE_X": hp.OUT_DISCHARGE_X, "HP_OUT_DISCHARGE_Y": hp.OUT_DISCHARGE_Y, "HP_OUT_VELOCITY_X": hp.OUT_VELOCITY_X,
            "HP_OUT_VELOCITY_Y": hp.OUT_VELOCITY_Y, "HP_OUT_FROUDE": hp.OUT_FROUDE, "HP_OUT_COUNT": hp.OUT_COUNT}
    assert enum == want and hp.OUT_COUNT == 9
    # every value name of the front end has a code, and the reference's substring order picks it
    assert sorted(hp.OUT_CODES.values()) == list(range(hp.OUT_COUNT))
    assert hp.OUT_CODES[frontend.data_value_code("MaxDepth")] == hp.OUT_MAXDEPTH
    assert hp.OUT_CODES[frontend.data_value_code("maxfsl")] == hp.OUT_MAXFSL
    assert "hp_domain_derive" in hp.EXPORTS and "hp_domain_stats" in hp.EXPORTS
    # the struct: field order and size as declared
    body = re.search(r"typedef struct \{([^}]*)\}\s*hp_domain_stats_t;", code).group(1)
    fields = re.findall(r"\b(\w+)\s*;", body)
    assert fields == [f[0] for f in hp.DomainStats._fields_] and C.sizeof(hp.DomainStats) == 64
    lib = hp.load_library()
    assert lib.hp_abi_version() == 2                                    # new symbols only


def test_argument_errors_are_error_codes_without_a_gpu():
    """The checks that do not need the domain come before the NULL-domain test, so each of them is reached here; with good
    arguments the NULL domain is the error.  (The row range needs a domain: tests/test_gpu_output_stage.py.)"""
    lib = hp.load_library()
    buf = np.zeros(16)
    good_values, good_rasters = (C.c_int * 2)(hp.OUT_DEPTH, hp.OUT_FSL), (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    cases = [
        ((good_values, 2, 8, good_rasters), "null domain"),
        ((good_values, 0, 8, good_rasters), "count outside"),
        ((good_values, -3, 8, good_rasters), "count outside"),
        ((good_values, hp.OUT_COUNT + 1, 8, good_rasters), "count outside"),
        ((None, 2, 8, good_rasters), "values / rasters == NULL"),
        ((good_values, 2, 8, None), "values / rasters == NULL"),
        ((good_values, 2, 0, good_rasters), "element_bytes"),
        ((good_values, 2, 2, good_rasters), "element_bytes"),
        ((good_values, 2, 16, good_rasters), "element_bytes"),
        (((C.c_int * 2)(hp.OUT_DEPTH, hp.OUT_COUNT), 2, 8, good_rasters), "unknown value 9"),
        (((C.c_int * 2)(-1, hp.OUT_DEPTH), 2, 8, good_rasters), "unknown value -1"),
        (((C.c_int * 2)(hp.OUT_FROUDE, hp.OUT_FROUDE), 2, 8, good_rasters), "value 8 listed twice"),
        ((good_values, 2, 8, (C.c_void_p * 2)(buf.ctypes.data, None)), "rasters[1] == NULL"),
        ((good_values, 2, 4, (C.c_void_p * 2)(None, buf.ctypes.data)), "rasters[0] == NULL"),
    ]
    for args, message in cases:
        assert lib.hp_domain_derive(None, *args, 0, 1) == -1, message           # HP_ERR_INVALID
        assert message.encode() in lib.hp_last_error(), (message, lib.hp_last_error())
    assert lib.hp_domain_derive(None, *cases[0][0], 0, 0) == -1                 # nrows == 0 does not excuse a NULL domain
    stats = hp.DomainStats()
    stats.struct_size = C.sizeof(hp.DomainStats)
    assert lib.hp_domain_stats(None, 0, 1, C.byref(stats)) == -1 and b"null domain" in lib.hp_last_error()
    assert lib.hp_domain_stats(None, 0, 1, None) == -1 and b"out == NULL" in lib.hp_last_error()
    for size in (0, 56, 72):
        stats.struct_size = size
        assert lib.hp_domain_stats(None, 0, 1, C.byref(stats)) == -1 and b"size mismatch" in lib.hp_last_error()


def test_unknown_names_are_rejected_before_the_library_is_called():
    dom = hp.Domain.__new__(hp.Domain)          # no device: derive() must fail on the name alone
    dom.rows, dom.cols, dom.h = 4, 4, None
    for name in ("dem", "manningcoefficient", "x"):
        with pytest.raises(ValueError, match="unknown output"):
            dom.derive([name])
    with pytest.raises(ValueError, match="dtype"):
        dom.derive(["depth"], dtype=np.int32)


def test_strip_statistics_combine_exactly():
    a = dict(cells=10, cells_wet=4, volume=1.5, max_depth=2.0, max_speed=0.5, max_depth_cell=7, max_speed_cell=3)
    b = dict(cells=12, cells_wet=0, volume=0.25, max_depth=2.0, max_speed=0.0, max_depth_cell=1, max_speed_cell=None)
    c = dict(cells=5, cells_wet=5, volume=0.125, max_depth=3.0, max_speed=0.5, max_depth_cell=2, max_speed_cell=0)
    out = strips.combine_stats([a, b, c], [0, 9, 19], cols=10)
    assert (out["cells"], out["cells_wet"], out["volume"]) == (27, 9, (1.5 + 0.25) + 0.125)
    assert (out["max_depth"], out["max_depth_cell"]) == (3.0, 2 + 19 * 10)
    assert (out["max_speed"], out["max_speed_cell"]) == (0.5, 3)          # the tie goes to the lowest global id
    dry = strips.combine_stats([b], [0], cols=10)
    assert dry["max_speed_cell"] is None and dry["max_speed"] == 0.0
    parts = [{"depth": np.ones((2, 3))}, {"depth": np.zeros((1, 3))}]
    assert strips.assemble_outputs(parts)["depth"].shape == (3, 3)


def _oracle_sim(cfg, cols, rows, res):
    return oracle.OracleSim(cols, rows, dx=res, scheme=cfg.scheme, very_small=cfg.dry_threshold, courant=cfg.courant,
                            end_time=cfg.duration, friction=cfg.friction, threads=4)


def test_model_over_an_engine_without_derive_takes_the_host_path(tmp_path):
    from hipims_mi.model import Model
    xml = make_newcastle(tmp_path, duration=60, frequency=30)
    lines = []
    m = Model(xml, make_sim=_oracle_sim, log=lines.append)
    assert m.device_outputs is False and not hasattr(m.sim, "derive")
    m.scheme.automatic_queue = False
    m.scheme.queue_addition_size = 50
    outs = m.run()
    assert [round(t, 6) for t, _ in outs] == [30.0, 60.0]
    final = m.sim.download()
    for what, _ in m.cfg.targets:                                       # today's derivation of the final state
        assert np.array_equal(outs[-1][1][what], frontend.derive_output(what, final, m.bed, m.res))
    assert m.domain_stats == [] and not any("domain volume" in l.lower() for l in lines)   # no stats() on this engine
    assert set(m.progress_blocks[-1]) == {"simulation_time", "lowest_timestep", "cells_calculated", "rate", "processing_time",
                                          "remaining", "batch_size", "progress"}
    with pytest.raises(ValueError, match="derive"):
        Model(xml, make_sim=_oracle_sim, device_outputs=True)


def test_default_output_path_by_precision(tmp_path):
    """An engine with derive(): the device path is the default for fp64 domains only (an fp32 domain's device bed is not the
    front end's fp64 bed, so its rasters would differ from the host derivation's); True / False force a path."""
    from hipims_mi.model import Model

    class WithDerive(oracle.OracleSim):
        def derive(self, values, **kw):
            raise AssertionError("not called here")

    def make(cfg, cols, rows, res):
        return WithDerive(cols, rows, dx=res, scheme=cfg.scheme, very_small=cfg.dry_threshold, courant=cfg.courant,
                          end_time=cfg.duration, friction=cfg.friction, threads=4)

    xml = make_newcastle(tmp_path, duration=60, frequency=30)
    assert Model(xml, make_sim=make).device_outputs is True
    assert Model(xml, make_sim=make, device_outputs=False).device_outputs is False
    text = open(xml).read().replace('value="double"', 'value="single"')
    open(xml, "w").write(text)
    assert Model(xml, make_sim=make).cfg.precision == "f32"
    assert Model(xml, make_sim=make).device_outputs is False
    assert Model(xml, make_sim=make, device_outputs=True).device_outputs is True
