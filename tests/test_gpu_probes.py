"""The probe recorder on the device (hp_probes_*; csrc/hp_probes.hpp: record_probes) against its NumPy restatement
(frontend.ProbeRecorder) fed the downloaded state and the device's time at every sample -- bit for bit: every operation is a
correctly rounded one and the order of every sum is fixed, so there are no tolerances.  GPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hipims_mi as hp
from hipims_mi import frontend, synthetic as syn
from test_gpu_output_stage import doctor

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES = (3, 4, 5, 2, 1, 8)               # batches of pairs and of single iterations
ND = frontend.NODATA
DX = 2.5
SECTION_LENGTHS = (2, 255, 256, 257, 513)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def probe_set(cols, rows, gauge_count, seed):
    """Gauges: a doctored wall cell (0, 0), the doctored disabled cell (1, 1) and a duplicate where the count allows, random cells
    otherwise.  Sections: one of each length of SECTION_LENGTHS with random cells (revisited) and random weights, the rasterised
    diagonal of the grid, and one along row 0 -- a closed-edge wall once the state is doctored: uncounted cells only."""
    rng = np.random.default_rng(seed)
    inner = (int(rng.integers(1, cols - 1)), int(rng.integers(1, max(2, rows - 1))))
    fixed = [inner, (0, 0), (1, 1), inner][:gauge_count]
    more = gauge_count - len(fixed)
    gauges = fixed + list(zip(rng.integers(0, cols, more).tolist(), rng.integers(0, rows, more).tolist()))
    sections = []
    for m in SECTION_LENGTHS:
        cells = np.stack([rng.integers(0, cols, m), rng.integers(0, rows, m)], axis=1)
        sections.append(frontend.Section(cells, rng.integers(-1, 2, m).astype(np.int8), rng.integers(-1, 2, m).astype(np.int8)))
    sections.append(frontend.rasterise_section((1, 1), (cols - 2, rows - 2)))
    dead = frontend.rasterise_section((cols - 1, 0), (0, 0))
    sections.append(frontend.Section(dead.cells, np.ones(cols, np.int8), np.ones(cols, np.int8)))
    return gauges, sections


def assert_series(got, want):
    for key in ("t", "gauges", "sections"):
        assert got[key].dtype == np.float64 and got[key].shape == want[key].shape, key
        assert not np.isnan(got[key]).any(), key
        assert np.array_equal(bits(got[key]), bits(want[key])), (key, int((bits(got[key]) != bits(want[key])).sum()))


def recorded_run(cols, rows, precision, gauge_count, scheme=hp.SCHEME_GODUNOV, seed=7, capacity=4096):
    """S-ROUGH, six samples after BATCHES, the doctored state uploaded before the third.  -> (domain, host recorder)"""
    real = np.float64 if precision == "f64" else np.float32
    st, bed, man = syn.s_rough(cols, rows, seed=seed, dtype=real)
    dom = hp.Domain(cols, rows, dx=DX, scheme=scheme, precision=precision)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    gauges, sections = probe_set(cols, rows, gauge_count, seed)
    dom.probes_enable(gauges, sections, capacity=capacity)
    ref = frontend.ProbeRecorder(gauges, sections, dx=DX)
    for k, n in enumerate(BATCHES):
        dom.step_batch(n)
        if k == 2:
            st2, bed = doctor(dom.download(), bed)
            dom.upload(st2, bed, None)                  # (does not touch the recorder)
        dom.probes_sample()
        ref.record(dom.download(), bed, dom.read_scalars()["time"])
    return dom, ref


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("size,gauge_count", [((67, 45), 257), ((64, 3), 1), ((257, 130), 256)])
def test_device_record_equals_the_host_recorder(size, gauge_count, precision):
    cols, rows = size
    dom, ref = recorded_run(cols, rows, precision, gauge_count, seed=400 + cols)
    got, want = dom.probes(), ref.series()
    assert_series(got, want)
    info = dom.probes_info()
    assert info == dict(samples=len(BATCHES), pending=len(BATCHES), capacity=4096, stride=1 + 4 * gauge_count + len(SECTION_LENGTHS) + 2)
    assert (np.diff(got["t"]) > 0).all()
    assert (got["gauges"][:, 0] != ND).all()                                       # an inner cell: counted in every sample
    if gauge_count >= 4:
        assert (got["gauges"][3:, 1:3] == ND).all() and np.array_equal(got["gauges"][:, 0], got["gauges"][:, 3])   # wall, disabled; the duplicate
    if rows > 3:                                                                   # (on three rows doctor's later edits land on the wall row)
        assert np.array_equal(bits(got["sections"][3:, -1]), bits(np.zeros(3)))    # uncounted cells only: +0.0
        assert (got["sections"][:, 1:-1] != 0).any(axis=0).all()                   # every long section carries water
    dom.close()


@pytest.mark.parametrize("scheme", [hp.SCHEME_MUSCL_HANCOCK, hp.SCHEME_INERTIAL])
def test_device_record_equals_the_host_recorder_other_schemes(scheme):
    dom, ref = recorded_run(67, 45, "f64", 5, scheme=scheme, seed=11)
    assert_series(dom.probes(), ref.series())
    dom.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [hp.MATH_FAST, hp.MATH_STRICT])
def test_recording_does_not_perturb_the_run(mode):
    cols, rows = 257, 130
    st, bed, man = syn.s_rough(cols, rows, seed=3)
    gauges, sections = probe_set(cols, rows, 9, 3)
    seen = []
    for recorded in (False, True):
        dom = hp.Domain(cols, rows, math_mode=mode)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        if recorded:
            dom.probes_enable(gauges, sections)
        for _ in range(8):
            dom.step_batch(8)
            if recorded:
                dom.probes_sample()
        ps = dom.pair_stats()
        seen.append((dom.download(), dom.read_scalars(), dom.launch_counts(), (ps["pairs"], ps["skipped_rows"], ps["still_rows"])))
        if recorded:
            assert dom.probes_info()["samples"] == 8 and dom.probes()["t"][-1] == seen[-1][1]["time"]
        dom.close()
    plain, recorded = seen
    assert np.array_equal(plain[0], recorded[0])
    assert plain[1] == recorded[1] and plain[1]["iterations"] == 64
    assert plain[2] == recorded[2] and plain[3] == recorded[3], (plain[2:], recorded[2:])


# 3 ---------------------------------------------------------------------------------------------------------------------
def raw_info(dom):
    n, cap, stride = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert dom.lib.hp_probes_info(dom.h, C.byref(n), C.byref(cap), C.byref(stride)) == 0
    return n.value, cap.value, stride.value


def test_capacity():
    cols, rows = 67, 45
    st, bed, man = syn.s_rough(cols, rows, seed=9)
    gauges, sections = probe_set(cols, rows, 3, 9)
    dom = hp.Domain(cols, rows, dx=DX)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.probes_enable(gauges, sections, capacity=3)
    lib = dom.lib
    for _ in range(3):
        dom.step_batch(2)
        assert lib.hp_probes_sample(dom.h) == 0
    assert lib.hp_probes_sample(dom.h) == -5 and b"full" in lib.hp_last_error()      # HP_ERR_STATE, nothing enqueued
    assert raw_info(dom) == (3, 3, 1 + 4 * 3 + len(sections))
    first = dom.probes()
    assert first["t"].shape == (3,)
    # Domain.probes_sample drains a full buffer by itself: seven samples come back in order
    dom.probes_enable(gauges, sections, capacity=3)
    ref = frontend.ProbeRecorder(gauges, sections, dx=DX)
    for k in range(7):
        dom.step_batch(k + 1)
        dom.probes_sample()
        ref.record(dom.download(), bed, dom.read_scalars()["time"])
    assert dom.probes_info() == dict(samples=7, pending=1, capacity=3, stride=1 + 4 * 3 + len(sections))
    assert_series(dom.probes(), ref.series())
    assert_series(dom.probes(), ref.series())                                      # (reading takes nothing away)
    dom.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_error_table():
    cols, rows = 64, 32
    st, bed, man = syn.s_rough(cols, rows, seed=2)
    dom = hp.Domain(cols, rows, dx=DX)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    lib = dom.lib
    cells = cols * rows
    gauges, sections = [(3, 4), (60, 30)], [frontend.rasterise_section((2, 2), (50, 20))]
    ref = [None]
    buf = np.zeros(64 * 64)
    out = buf.ctypes.data_as(C.POINTER(C.c_double))

    def goes_on():
        """The domain still steps -- and records, while the recorder is on."""
        dom.step_batch(3)
        if ref[0] is not None:
            dom.probes_sample()
            ref[0].record(dom.download(), bed, dom.read_scalars()["time"])
            assert_series(dom.probes(), ref[0].series())

    def fails(code, message, call):
        with pytest.raises(hp.HipimsError, match=rf"\({code}\).*{message}"):
            call()
        goes_on()

    def raw(rc, code, message):
        assert rc == code and message.encode() in lib.hp_last_error(), (rc, lib.hp_last_error())
        goes_on()

    good = (np.array([5, 6, 7]), [1, 0, -1], [0, 1, 0])
    for on in (False, True):                 # every argument error with the recorder off, then with it on (which it leaves as it was)
        fails(-1, "gauge 1: cell id outside", lambda: dom.probes_enable_cells([0, cells]))
        fails(-1, "section entry 2: cell id outside", lambda: dom.probes_enable_cells([0], [(np.array([5, 6, cells + 7]), good[1], good[2])]))
        fails(-1, "section entry 1: weight outside", lambda: dom.probes_enable_cells([], [(good[0], [1, 2, 0], good[2])]))
        fails(-1, "section entry 0: weight outside", lambda: dom.probes_enable_cells([], [(good[0], good[1], [-2, 0, 0])]))
        fails(-1, "section 1 is shorter than 2", lambda: dom.probes_enable_cells([1], [good, (np.array([9]), [1], [1])]))
        fails(-1, "256 MiB", lambda: dom.probes_enable_cells(np.arange(2048), capacity=4096))      # 4096 x 8193 x 8 B
        fails(-1, "capacity", lambda: dom.probes_enable_cells([1], capacity=0))
        fails(-1, "neither a gauge nor a section", lambda: dom.probes_enable_cells([]))
        g = np.array([1], np.uint64)
        desc = hp.ProbesDesc(C.sizeof(hp.ProbesDesc) - 8, 4, 1, g.ctypes.data_as(C.POINTER(C.c_uint64)), 0, None, None, None, None)
        raw(lib.hp_probes_enable(dom.h, C.byref(desc)), -1, "size mismatch")
        if not on:
            fails(-5, "hp_probes_sample before hp_probes_enable", dom.probes_sample)
            raw(lib.hp_probes_read(dom.h, 0, 1, out), -5, "hp_probes_read before hp_probes_enable")
            fails(-5, "hp_probes_info before hp_probes_enable", dom.probes_info)
            raw(lib.hp_probes_reset(dom.h), -5, "hp_probes_reset before hp_probes_enable")
            dom.probes_disable()                                                  # idempotent
            dom.probes_enable(gauges, sections, capacity=64)
            ref[0] = frontend.ProbeRecorder(gauges, sections, dx=DX)
            goes_on()
    n = raw_info(dom)[0]
    assert n >= 9
    raw(lib.hp_probes_read(dom.h, 0, n + 1, out), -1, "beyond the samples taken")
    raw(lib.hp_probes_read(dom.h, raw_info(dom)[0] + 1, 0, out), -1, "beyond the samples taken")
    raw(lib.hp_probes_read(dom.h, 1, 2 ** 64 - 1, out), -1, "beyond the samples taken")
    raw(lib.hp_probes_read(dom.h, 0, 1, None), -1, "records == NULL")
    assert lib.hp_probes_read(dom.h, raw_info(dom)[0], 0, None) == 0              # count == 0 is HP_OK
    # inside a split step
    dom.step_begin()
    before = raw_info(dom)[0]
    assert lib.hp_probes_sample(dom.h) == -5 and b"hp_probes_sample between hp_step_begin and hp_step_end" in lib.hp_last_error()
    assert lib.hp_probes_read(dom.h, 0, 1, out) == -5 and b"hp_probes_read between hp_step_begin and hp_step_end" in lib.hp_last_error()
    assert raw_info(dom)[0] == before
    dom.step_end()
    goes_on()
    # a partial read, queued behind the samples: records [2, 5)
    stride = raw_info(dom)[2]
    assert lib.hp_probes_read(dom.h, 2, 3, out) == 0
    dom.sync()
    want = ref[0].series()
    assert np.array_equal(buf[:3 * stride].reshape(3, stride)[:, 0], want["t"][2:5])
    assert np.array_equal(bits(buf[:3 * stride].reshape(3, stride)[:, -1]), bits(want["sections"][2:5, 0]))
    dom.probes_disable()
    dom.probes_disable()
    ref[0] = None
    fails(-5, "before hp_probes_enable", dom.probes_sample)
    dom.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_save_and_restore():
    cols, rows = 257, 130
    st, bed, man = syn.s_rough(cols, rows, seed=5)
    gauges, sections = probe_set(cols, rows, 7, 5)
    batches = (6, 7, 8, 5)
    dom = hp.Domain(cols, rows, dx=DX)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.probes_enable(gauges, sections, capacity=16)

    def advance(some):
        for n in some:
            dom.step_batch(n)
            dom.probes_sample()

    logs = []
    hp.set_log_sink(lambda level, text: logs.append((level, text)))
    try:
        advance(batches[:2])
        dom.state_save()
        advance(batches[2:])
        first, state = dom.probes(), dom.download()
        assert raw_info(dom)[0] == 4
        dom.state_restore()
        assert raw_info(dom)[0] == 2 and dom.probes_info()["samples"] == 2
        advance(batches[2:])
        assert np.array_equal(dom.download(), state)
        assert_series(dom.probes(), first)
        assert first["t"].shape == (4,) and not logs
        # a reset between save and restore: count 0, exactly one warning
        dom.state_save()
        advance((3,))
        assert dom.lib.hp_probes_reset(dom.h) == 0
        advance((2,))
        assert raw_info(dom)[0] == 1
        dom.state_restore()
        assert raw_info(dom)[0] == 0
        warnings = [text for level, text in logs if level == 8]
        assert len(warnings) == 1 and "probe sample count" in warnings[0], logs
        advance((4,))                                                             # ... and the recorder records on
        assert raw_info(dom)[0] == 1
        # with the recorder off a restore says nothing
        dom.probes_disable()
        dom.state_restore()
        assert len([1 for level, _ in logs if level == 8]) == 1
    finally:
        hp.set_log_sink(None)
    dom.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_strips_gather_probes(world):
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", lib,
                               os.path.join(os.path.dirname(lib), "fake_rccl.cpp")])
    res = subprocess.run([sys.executable, os.path.join(HERE, "probes_strips_worker.py"), str(world)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "probes bit-identical True" in res.stdout and "every section carries water True" in res.stdout


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_model_writes_the_same_files_from_the_device_and_from_the_host(tmp_path):
    from hipims_mi.model import Model
    from model_dir import make_newcastle
    files = {}
    for tag, device in (("device", True), ("host", False)):
        xml = make_newcastle(tmp_path / tag, duration=600, frequency=60)
        text = open(xml).read()
        marker = '<dataTarget type="raster" value="maxdepth" format="HFA" target="maxdepth_%t.img" />'
        assert marker in text
        open(xml, "w").write(text.replace(marker, marker + '\n<gauge name="quay" x="120" y="60"/>\n<gauge name="wall" x="0" y="7"/>'
                                          '\n<section name="street" x0="100" y0="80" x1="180" y1="110"/>'))
        m = Model(xml, output_format=".npy", device_outputs=device, probe_capacity=5)
        m.scheme.automatic_queue = False                                      # (batch boundaries are not physics-neutral: fixed)
        m.scheme.queue_addition_size = 16
        assert m.device_probes is device and (m.host_probes is None) is device
        m.run(max_outputs=2)
        series, samples = m.probes(), m.scheme.iterations // 16
        m.close()
        out = os.path.join(str(tmp_path / tag), "output")
        files[tag] = (open(os.path.join(out, "gauges.csv"), "rb").read(), open(os.path.join(out, "sections.csv"), "rb").read())
        assert series["t"].shape == (samples,) and samples > 5                # (the device buffer of 5 was drained on the way)
        assert files[tag][0].count(b"\n") == 1 + 2 * samples and files[tag][1].count(b"\n") == 1 + samples
    assert files["device"] == files["host"]
    assert files["host"][0].startswith(b"time,name,fsl,depth,qx,qy\n") and files["host"][1].startswith(b"time,name,discharge\n")
    assert b",wall,-9999.0,-9999.0,-9999.0,-9999.0\n" in files["host"][0]          # a closed-edge cell: not counted
    assert any(not line.endswith(b",0.0") for line in files["host"][1].splitlines()[1:])
