"""The peak tracker without a GPU: the six hp_peaks_* entry points and their argument checks, the NumPy restatement
(frontend.PeakTracker, the reference the GPU tests hold the device kernel to) on hand-made states, and a Model run with
peak targets on the oracle engine."""
import ctypes as C
import re

import numpy as np
import pytest

import hipims_mi as hp
import oracle
from hipims_mi import frontend
from model_dir import make_newcastle
from test_abi import HEADER, declared_functions

ND = frontend.NODATA
PEAK_FUNCTIONS = ["hp_peaks_disable", "hp_peaks_enable", "hp_peaks_info", "hp_peaks_read", "hp_peaks_reset", "hp_peaks_sample"]


def test_header_declares_and_library_exports_the_six_entry_points():
    lib = hp.load_library()
    assert [n for n in declared_functions() if n.startswith("hp_peaks_")] == PEAK_FUNCTIONS
    for n in PEAK_FUNCTIONS:
        assert hasattr(lib, n) and n in hp.EXPORTS
    text = open(HEADER).read()
    assert int(re.search(r"HP_PEAK_COUNT = (\d+)", text).group(1)) == hp.PEAK_COUNT == len(hp.PEAK_CODES) == 5
    for name, code in (("SPEED", 0), ("UNIT_DISCHARGE", 1), ("HAZARD", 2), ("ARRIVAL_TIME", 3), ("WET_DURATION", 4)):
        assert re.search(rf"HP_PEAK_{name} = {code}\b", text) and getattr(hp, "PEAK_" + name) == code
    assert "#define HP_ABI_VERSION 2" in text and lib.hp_abi_version() == 2
    assert "no reference counterpart; closest: the Zmax field,\n *      CLSchemeGodunov.clc" in text
    assert C.sizeof(hp.PeaksDesc) == 16
    assert list(frontend.PEAK_NAMES) == sorted(hp.PEAK_CODES, key=hp.PEAK_CODES.get)


def test_argument_errors_come_before_any_device_use():
    lib = hp.load_library()

    def invalid(rc, message):
        assert rc == -1, (rc, message)
        assert message.encode() in lib.hp_last_error(), (message, lib.hp_last_error())

    def desc(size=C.sizeof(hp.PeaksDesc), mask=0b11111, arrival=0.01):
        return C.byref(hp.PeaksDesc(size, mask, arrival))

    invalid(lib.hp_peaks_enable(None, None), "desc == NULL")
    invalid(lib.hp_peaks_enable(None, desc(size=12)), "size mismatch")
    invalid(lib.hp_peaks_enable(None, desc(mask=0)), "values_mask is empty")
    invalid(lib.hp_peaks_enable(None, desc(mask=1 << 5)), "unknown value")
    invalid(lib.hp_peaks_enable(None, desc(arrival=9.9e-9)), "arrival_depth")
    invalid(lib.hp_peaks_enable(None, desc(arrival=float("nan"))), "arrival_depth")
    invalid(lib.hp_peaks_enable(None, desc(arrival=1e-8)), "null domain")            # 1e-8 itself is allowed
    invalid(lib.hp_peaks_enable(None, desc()), "null domain")
    for f in (lib.hp_peaks_disable, lib.hp_peaks_reset, lib.hp_peaks_sample):
        invalid(f(None), "null domain")
    n, t = C.c_uint64(0), C.c_double(0.0)
    invalid(lib.hp_peaks_info(None, C.byref(n), C.byref(t), C.byref(t)), "null domain")

    buf = np.zeros((4, 5))
    ok_values, ok_rasters = (C.c_int * 2)(hp.PEAK_SPEED, hp.PEAK_HAZARD), (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    for args, message in [
            ((ok_values, 0, 8, ok_rasters, 0, 4), "count outside"),
            ((ok_values, hp.PEAK_COUNT + 1, 8, ok_rasters, 0, 4), "count outside"),
            ((None, 2, 8, ok_rasters, 0, 4), "== NULL"),
            ((ok_values, 2, 8, None, 0, 4), "== NULL"),
            ((ok_values, 2, 2, ok_rasters, 0, 4), "element_bytes"),
            ((ok_values, 2, 16, ok_rasters, 0, 4), "element_bytes"),
            (((C.c_int * 2)(hp.PEAK_SPEED, hp.PEAK_COUNT), 2, 8, ok_rasters, 0, 4), "unknown value 5"),
            (((C.c_int * 2)(-1, hp.PEAK_SPEED), 2, 8, ok_rasters, 0, 4), "unknown value -1"),
            (((C.c_int * 2)(hp.PEAK_HAZARD, hp.PEAK_HAZARD), 2, 8, ok_rasters, 0, 4), "listed twice"),
            ((ok_values, 2, 8, (C.c_void_p * 2)(buf.ctypes.data, None), 0, 4), "rasters[1] == NULL"),
            ((ok_values, 2, 8, ok_rasters, 0, 4), "null domain")]:
        invalid(lib.hp_peaks_read(None, *args), message)


def test_names():
    assert [frontend.peak_value_code(n) for n in ("peakSpeed", "PeakUnitDischarge", " hazard", "arrivalTime", "wetduration")] == \
        list(frontend.PEAK_NAMES)
    for n in ("speed", "maxdepth", "depth", "", None, "hazard_final"):
        assert frontend.peak_value_code(n) is None
    for n in frontend.PEAK_NAMES:                      # a target is an output raster or a peak, never both
        assert frontend.data_value_code(n) is None


def test_peak_tracker_on_hand_made_states():
    cols, rows = 5, 4
    above = np.nextafter(0.01, 1.0)
    bed = np.zeros((rows, cols))
    s = [np.zeros((rows, cols, 4)) for _ in range(3)]

    def put(cell, zb, samples):
        bed.reshape(-1)[cell] = zb
        for k, v in enumerate(samples):
            s[k].reshape(-1, 4)[cell] = v

    # cell 6: wets, dries, wets again (depth 0.5 with v = 5, dry, depth 0.25 with v = 10)
    put(6, 1.0, [(1.5, 1.5, 1.5, 2.0), (1.0, 1.5, 0.0, 0.0), (1.25, 1.5, 1.5, 2.0)])
    # cell 7: exactly at the arrival depth, at rest;  cell 8: one ulp above it
    put(7, 0.0, [(0.01, 0.01, 0.0, 0.0)] * 3)
    put(8, 0.0, [(above, above, 0.0, 0.0)] * 3)
    # cell 11: disabled;  cell 12: a wall with water on it;  cell 13: Z < zb with a discharge
    put(11, 2.0, [(3.0, -9999.0, 1.0, 1.0)] * 3)
    put(12, 9999.9, [(10001.0, 10001.0, 1.0, 1.0)] * 3)
    put(13, 2.0, [(1.5, 1.5, 0.25, -0.25)] * 3)
    # cell 16: wet in the sample that repeats the time only (duration 0, not NODATA)
    put(16, 0.0, [(0.0, 0.0, 0.0, 0.0), (2.0, 2.0, 0.0, -4.0), (0.0, 2.0, 0.0, 0.0)])

    tr = frontend.PeakTracker(rows, cols, arrival_depth=0.01, t=0.0)
    for state, t in zip(s, (0.5, 0.5, 2.0)):
        tr.fold(state, bed, t)
    assert tr.info() == dict(samples=3, t_first=0.5, t_last=2.0)
    got = tr.rasters()

    def want(**cells):
        a = np.full(rows * cols, ND)
        for k, v in cells.items():
            a[int(k[1:])] = v
        return a.reshape(rows, cols)

    expected = dict(
        peakspeed=want(c6=10.0, c7=0.0, c8=0.0, c16=2.0),
        peakunitdischarge=want(c6=2.5, c7=0.0, c8=0.0, c16=4.0),
        hazard=want(c6=2.75, c7=0.005, c8=above * 0.5, c16=5.0),
        arrivaltime=want(c6=0.5, c8=0.5, c16=0.5),
        wetduration=want(c6=2.0, c8=2.0, c16=0.0))
    assert set(got) == set(expected) == set(frontend.PEAK_NAMES)
    for name in expected:
        assert got[name].dtype == np.float64 and np.array_equal(got[name], expected[name]), (name, got[name])
    # fp32 inputs are widened first: the same numbers where they are fp32 numbers
    tr32 = frontend.PeakTracker(rows, cols, arrival_depth=0.01, t=0.0)
    for state, t in zip(s, (0.5, 0.5, 2.0)):
        tr32.fold(state.astype(np.float32), bed.astype(np.float32), t)
    assert np.array_equal(tr32.rasters()["peakspeed"][1], expected["peakspeed"][1])
    # reset: NODATA everywhere, t_previous = t
    tr.reset(2.0)
    assert all((a == ND).all() for a in tr.rasters().values()) and tr.info() == dict(samples=0, t_first=2.0, t_last=2.0)
    tr.fold(s[0], bed, 3.0)
    assert tr.rasters()["wetduration"].reshape(-1)[6] == 1.0
    with pytest.raises(ValueError):
        frontend.PeakTracker(rows, cols, arrival_depth=1e-9)


def _oracle_sim(cfg, cols, rows, res):
    return oracle.OracleSim(cols, rows, dx=res, scheme=cfg.scheme, very_small=cfg.dry_threshold, courant=cfg.courant,
                            end_time=cfg.duration, friction=cfg.friction, threads=4)


def test_model_with_peak_targets_on_the_oracle_engine(tmp_path):
    from hipims_mi.model import Model
    runs = {}
    for tag in ("plain", "peaks"):
        xml = make_newcastle(tmp_path / tag, duration=600, frequency=30)
        if tag == "peaks":
            text = open(xml).read()
            marker = '<dataTarget type="raster" value="maxdepth" format="HFA" target="maxdepth_%t.img" />'
            assert marker in text
            open(xml, "w").write(text.replace(marker, marker + '\n<dataTarget type="raster" value="arrivalTime" format="HFA" '
                                              'target="arrival_%t.img" />\n<dataTarget type="raster" value="wetDuration" '
                                              'format="HFA" target="wet_%t.img" />'))
        m = Model(xml, make_sim=_oracle_sim, output_format=".npy", peak_arrival_depth=0.0002)
        m.scheme.automatic_queue = False                   # (batch boundaries are not physics-neutral: fixed)
        m.scheme.queue_addition_size = 25
        calls = []
        if tag == "plain":
            assert m.scheme.peak_sampler is None and m.peak_names == [] and m.host_peaks is None
        else:
            assert m.peak_names == ["arrivaltime", "wetduration"] and m.host_peaks is not None and not m.device_peaks
            sampler = m.scheme.peak_sampler
            m.scheme.peak_sampler = lambda: (calls.append(1), sampler())[1]
        outs = m.run(max_outputs=2)
        runs[tag] = (outs, m.sim.download(), m.sim.scalars(), len(calls), m.scheme.iterations)
        m.close()
    plain, peaks = runs["plain"], runs["peaks"]
    assert [t for t, _ in plain[0]] == [t for t, _ in peaks[0]] == [30.0, 60.0]
    assert peaks[3] > 0 and peaks[3] * 25 == peaks[4]      # one sample after every batch queued
    assert np.array_equal(plain[1], peaks[1]) and plain[2] == peaks[2]
    for (t, a), (_, b) in zip(plain[0], peaks[0]):
        assert set(b) == set(a) | {"arrivaltime", "wetduration"}
        for name in a:                                     # every non-peak raster: the same bits
            assert np.array_equal(a[name], b[name]), name
        arrival, wet = b["arrivaltime"], b["wetduration"]
        assert arrival.dtype == wet.dtype == np.float64 and arrival.shape == wet.shape == (195, 342)
        assert np.array_equal(arrival == ND, wet == ND)
        reached = arrival != ND
        assert reached.any() and not reached.all()         # rain has filled some cells past the arrival depth; the walls never
        assert (arrival[reached] >= 0.0).all() and (arrival[reached] <= t).all()
        assert (wet[reached] >= 0.0).all() and (wet[reached] <= t).all()
    import os
    files = sorted(os.listdir(os.path.join(str(tmp_path / "peaks"), "output")))
    assert "arrival_30.npy" in files and "wet_60.npy" in files and len(files) == 14
    assert np.array_equal(np.load(os.path.join(str(tmp_path / "peaks"), "output", "wet_60.npy")), peaks[0][-1][1]["wetduration"])
    # Model(peaks=[...]) without a target: tracked and returned, no file
    xml = make_newcastle(tmp_path / "kw", duration=600, frequency=30)
    m = Model(xml, make_sim=_oracle_sim, output_format=".npy", peaks=["hazard"])
    m.scheme.automatic_queue = False
    m.scheme.queue_addition_size = 25
    outs = m.run(max_outputs=1)
    m.close()
    assert "hazard" in outs[0][1] and len(os.listdir(os.path.join(str(tmp_path / "kw"), "output"))) == 5
    with pytest.raises(ValueError, match="unknown peak value"):
        Model(xml, make_sim=_oracle_sim, peaks=["speed"])
