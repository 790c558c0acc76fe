"""The zone recorder on the device (hp_zones_*; csrc/hp_zones.hpp: record_zones) against its NumPy restatement
(frontend.ZoneRecorder) fed the downloaded state and the device's time at every sample -- word for word: everything the kernel
accumulates is an integer, so there are no tolerances, whatever the order in which the atomics arrive.  GPU only."""
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
BATCHES = (3, 4, 5, 2, 1, 8)               # batches of pairs and of single iterations (test_gpu_probes.py's)
DX = 2.5
FLOOD = 0.1
LAYOUTS = ("blocks", "stripes", "checkerboard", "random", "one", "sparse4096")
P64 = C.POINTER(C.c_uint64)


def layout(name, cols, rows, seed=0):
    """-> (ids[rows, cols], zone_count): id rasters that reach every path of the kernel."""
    y, x = np.mgrid[0:rows, 0:cols]
    if name == "blocks":                     # rectangles: long runs of one id, a change of id inside a row and between rows
        return 1 + (y * 3 // rows) * 4 + (x * 4 // cols), 12
    if name == "stripes":                    # widths 2, 1, 63, 64, 65, ...: a border at every kind of lane offset
        edges = np.cumsum(np.resize([2, 1, 63, 64, 65], cols))
        column = 1 + np.searchsorted(edges, np.arange(cols), side="right")
        return np.broadcast_to(column, (rows, cols)).copy(), int(column.max())
    if name == "checkerboard":               # every wave mixed: the per-lane path alone
        return 1 + (x + y) % 2, 2
    if name == "random":                     # independent ids per cell, 0 included
        return np.random.default_rng(seed).integers(0, 9, (rows, cols)), 8
    if name == "one":                        # one zone over everything, the doctored wall and disabled cells included
        return np.ones((rows, cols), int), 1
    if name == "sparse4096":                 # most ids unused: their records stay all-zero
        return np.choose((y * 2 // rows) * 2 + (x * 2 // cols), [0, 1, 2048, 4096]), 4096
    raise KeyError(name)


def assert_words(got, want):
    assert got.dtype == np.uint64 and got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (len(bad), [(int(i), int(j), (int(j) - 1) // 7 + 1, (int(j) - 1) % 7, int(got[i, j]), int(want[i, j])) for i, j in bad[:5]])


def recorded_run(cols, rows, precision, ids, zone_count, scheme=hp.SCHEME_GODUNOV, seed=7, capacity=4096):
    """S-ROUGH, six samples after BATCHES, the doctored state uploaded before the third.  -> (domain, host recorder)"""
    real = np.float64 if precision == "f64" else np.float32
    st, bed, man = syn.s_rough(cols, rows, seed=seed, dtype=real)
    dom = hp.Domain(cols, rows, dx=DX, scheme=scheme, precision=precision)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.zones_enable(ids, zone_count, flood_depth=FLOOD, capacity=capacity)
    ref = frontend.ZoneRecorder(ids, zone_count, FLOOD, DX)
    for k, n in enumerate(BATCHES):
        dom.step_batch(n)
        if k == 2:
            st2, bed = doctor(dom.download(), bed)
            dom.upload(st2, bed, None)                  # (does not touch the recorder)
        dom.zones_sample()
        ref.record(dom.download(), bed, dom.read_scalars()["time"])
    return dom, ref


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("size", [(67, 45), (64, 3), (257, 130)])
def test_device_record_equals_the_host_recorder(size, name, precision):
    cols, rows = size
    ids, zone_count = layout(name, cols, rows, seed=cols)
    capacity = 4096 if zone_count < 4096 else 8          # (4096 records of 4096 zones would be 896 MiB: over the 256 MiB limit)
    dom, ref = recorded_run(cols, rows, precision, ids, zone_count, seed=400 + cols, capacity=capacity)
    got, want = dom.zone_records(), ref.words()
    assert_words(got, want)
    assert dom.zones_info() == dict(samples=len(BATCHES), pending=len(BATCHES), capacity=capacity, stride=1 + 7 * zone_count)
    s, w = dom.zones(), ref.series()
    for key in w:
        assert s[key].dtype == w[key].dtype and np.array_equal(s[key].view(np.uint64), w[key].view(np.uint64)), key
    assert (np.diff(s["t"]) > 0).all() and not np.isnan(s["max_speed"]).any()
    present = np.unique(ids[ids > 0]) - 1
    absent = np.setdiff1d(np.arange(zone_count), present)
    assert not got[:, 1:].reshape(len(BATCHES), zone_count, 7)[:, absent].any()      # zones no cell carries stay all-zero
    if rows > 3 and name != "stripes":         # (on 67 columns the last stripe is the east wall alone: no counted cell)
        assert (s["wet"][:, present] > 0).all() and (s["volume"][:, present] > 0).all()   # every zone carries water
    if name == "one" and rows > 3:             # the doctored walls and the disabled cell are not counted; the device's own statistics agree
        assert 0 < s["cells"][-1, 0] < (cols - 2) * (rows - 2)
        st = dom.stats()
        assert (st["cells"], st["cells_wet"], st["max_depth"], st["max_speed"]) == \
            (int(s["cells"][-1, 0]), int(s["wet"][-1, 0]), s["max_depth"][-1, 0], s["max_speed"][-1, 0])
        assert abs(s["volume"][-1, 0] - st["volume"]) <= st["cells"] * DX * DX * 2.0 ** -33 + st["cells"] * 2.0 ** -52 * st["volume"]
    dom.close()


@pytest.mark.parametrize("name", ["blocks", "stripes", "random"])
def test_a_grid_on_which_a_wave_walks_several_steps(name):
    """Above 2048 x 256 cells a wave owns more than 64 cells and keeps a zone's figures in registers from step to step: the carry,
    the flush at a change of id between two steps and the last wave's short run are reached only here."""
    cols, rows = 1101, 997
    ids, zone_count = layout(name, cols, rows, seed=5)
    st, bed, man = syn.s_rough(cols, rows, seed=21)
    dom = hp.Domain(cols, rows, dx=DX)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.step_batch(6)
    st2, bed = doctor(dom.download(), bed)
    dom.upload(st2, bed, None)
    dom.zones_enable(ids, zone_count, flood_depth=FLOOD, capacity=2)
    ref = frontend.ZoneRecorder(ids, zone_count, FLOOD, DX)
    dom.zones_sample()
    ref.record(st2, bed, dom.read_scalars()["time"])
    assert_words(dom.zone_records(), ref.words())
    assert ref.words()[0, 1::7].all()                                              # every zone has counted cells
    dom.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [hp.SCHEME_MUSCL_HANCOCK, hp.SCHEME_INERTIAL])
def test_device_record_equals_the_host_recorder_other_schemes(scheme):
    ids, zone_count = layout("blocks", 67, 45)
    dom, ref = recorded_run(67, 45, "f64", ids, zone_count, scheme=scheme, seed=11)
    assert_words(dom.zone_records(), ref.words())
    dom.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [hp.MATH_FAST, hp.MATH_STRICT])
def test_recording_does_not_perturb_the_run(mode):
    cols, rows = 257, 130
    st, bed, man = syn.s_rough(cols, rows, seed=3)
    ids, zone_count = layout("stripes", cols, rows)
    seen = []
    for recorded in (False, True):
        dom = hp.Domain(cols, rows, math_mode=mode)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        if recorded:
            dom.zones_enable(ids, zone_count)
        for _ in range(8):
            dom.step_batch(8)
            if recorded:
                dom.zones_sample()
        ps = dom.pair_stats()
        seen.append((dom.download(), dom.read_scalars(), dom.launch_counts(), (ps["pairs"], ps["skipped_rows"], ps["still_rows"])))
        if recorded:
            assert dom.zones_info()["samples"] == 8 and dom.zones()["t"][-1] == seen[-1][1]["time"]
        dom.close()
    plain, recorded = seen
    assert np.array_equal(plain[0], recorded[0])
    assert plain[1] == recorded[1] and plain[1]["iterations"] == 64
    assert plain[2] == recorded[2] and plain[3] == recorded[3], (plain[2:], recorded[2:])


# 4 ---------------------------------------------------------------------------------------------------------------------
def raw_info(dom):
    n, cap, stride = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert dom.lib.hp_zones_info(dom.h, C.byref(n), C.byref(cap), C.byref(stride)) == 0
    return n.value, cap.value, stride.value


def test_capacity_and_reset():
    cols, rows = 67, 45
    st, bed, man = syn.s_rough(cols, rows, seed=9)
    ids, zone_count = layout("blocks", cols, rows)
    dom = hp.Domain(cols, rows, dx=DX)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.zones_enable(ids, zone_count, capacity=3)
    lib = dom.lib
    for _ in range(3):
        dom.step_batch(2)
        assert lib.hp_zones_sample(dom.h) == 0
    assert lib.hp_zones_sample(dom.h) == -5 and b"full" in lib.hp_last_error()       # HP_ERR_STATE, nothing enqueued
    assert raw_info(dom) == (3, 3, 1 + 7 * zone_count)
    assert dom.zones()["t"].shape == (3,)
    # reset: count 0, and the slots are recorded afresh (a record is filled before it is added to)
    dom.zones_reset()
    assert raw_info(dom)[0] == 0 and dom.zones()["t"].shape == (0,)
    ref = frontend.ZoneRecorder(ids, zone_count, FLOOD, DX)
    dom.step_batch(3)
    dom.zones_sample()
    ref.record(dom.download(), bed, dom.read_scalars()["time"])
    assert_words(dom.zone_records(), ref.words())
    # Domain.zones_sample drains a full buffer by itself: seven samples come back in order
    dom.zones_enable(ids, zone_count, capacity=3)
    ref = frontend.ZoneRecorder(ids, zone_count, FLOOD, DX)
    for k in range(7):
        dom.step_batch(k + 1)
        dom.zones_sample()
        ref.record(dom.download(), bed, dom.read_scalars()["time"])
    assert dom.zones_info() == dict(samples=7, pending=1, capacity=3, stride=1 + 7 * zone_count)
    assert_words(dom.zone_records(), ref.words())
    assert_words(dom.zone_records(), ref.words())                                  # (reading takes nothing away)
    dom.close()


def test_error_table():
    cols, rows = 64, 32
    st, bed, man = syn.s_rough(cols, rows, seed=2)
    dom = hp.Domain(cols, rows, dx=DX)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    lib = dom.lib
    ids, zone_count = layout("blocks", cols, rows)
    ids16 = np.ascontiguousarray(ids, np.uint16)
    ref = [None]
    buf = np.zeros(64 * (1 + 7 * zone_count), np.uint64)
    out = buf.ctypes.data_as(P64)

    def goes_on():
        """The domain still steps -- and records, while the recorder is on."""
        dom.step_batch(3)
        if ref[0] is not None:
            dom.zones_sample()
            ref[0].record(dom.download(), bed, dom.read_scalars()["time"])
            assert_words(dom.zone_records(), ref[0].words())

    def fails(code, message, call):
        with pytest.raises(hp.HipimsError, match=rf"\({code}\).*{message}"):
            call()
        goes_on()

    def raw(rc, code, message):
        assert rc == code and message.encode() in lib.hp_last_error(), (rc, lib.hp_last_error())
        goes_on()

    bad = ids16.copy()
    bad.reshape(-1)[[77, 900]] = zone_count + 1
    for on in (False, True):                 # every argument error with the recorder off, then with it on (which it leaves as it was)
        fails(-1, f"cell 77: zone id {zone_count + 1} above zone_count", lambda: dom.zones_enable_raw(bad, zone_count))
        fails(-1, "zone_count outside 1..4096", lambda: dom.zones_enable_raw(np.zeros_like(ids16), 0))
        fails(-1, "zone_count outside 1..4096", lambda: dom.zones_enable_raw(ids16, 4097))
        fails(-1, "flood_depth must be at least 1e-8", lambda: dom.zones_enable_raw(ids16, zone_count, flood_depth=0.5e-8))
        fails(-1, "256 MiB", lambda: dom.zones_enable_raw(ids16, 4096, capacity=1171))     # 1171 x 28673 x 8 B
        fails(-1, "capacity", lambda: dom.zones_enable_raw(ids16, zone_count, capacity=0))
        desc = hp.ZonesDesc(C.sizeof(hp.ZonesDesc) - 8, 4, zone_count, 0, ids16.ctypes.data_as(C.POINTER(C.c_uint16)), FLOOD)
        raw(lib.hp_zones_enable(dom.h, C.byref(desc)), -1, "size mismatch")
        desc = hp.ZonesDesc(C.sizeof(hp.ZonesDesc), 4, zone_count, 0, None, FLOOD)
        raw(lib.hp_zones_enable(dom.h, C.byref(desc)), -1, "zone_of_cell == NULL")
        raw(lib.hp_zones_enable(dom.h, None), -1, "desc == NULL")
        if not on:
            fails(-5, "hp_zones_sample before hp_zones_enable", dom.zones_sample)
            raw(lib.hp_zones_read(dom.h, 0, 1, out), -5, "hp_zones_read before hp_zones_enable")
            fails(-5, "hp_zones_info before hp_zones_enable", dom.zones_info)
            raw(lib.hp_zones_reset(dom.h), -5, "hp_zones_reset before hp_zones_enable")
            dom.zones_disable()                                                   # idempotent
            dom.zones_enable(ids, zone_count, flood_depth=FLOOD, capacity=64)
            ref[0] = frontend.ZoneRecorder(ids, zone_count, FLOOD, DX)
            goes_on()
    n = raw_info(dom)[0]
    assert n >= 10
    raw(lib.hp_zones_read(dom.h, 0, n + 1, out), -1, "beyond the samples taken")
    raw(lib.hp_zones_read(dom.h, raw_info(dom)[0] + 1, 0, out), -1, "beyond the samples taken")
    raw(lib.hp_zones_read(dom.h, 1, 2 ** 64 - 1, out), -1, "beyond the samples taken")
    raw(lib.hp_zones_read(dom.h, 0, 1, None), -1, "records == NULL")
    assert lib.hp_zones_read(dom.h, raw_info(dom)[0], 0, None) == 0               # count == 0 is HP_OK
    # inside a split step
    dom.step_begin()
    before = raw_info(dom)[0]
    assert lib.hp_zones_sample(dom.h) == -5 and b"hp_zones_sample between hp_step_begin and hp_step_end" in lib.hp_last_error()
    assert lib.hp_zones_read(dom.h, 0, 1, out) == -5 and b"hp_zones_read between hp_step_begin and hp_step_end" in lib.hp_last_error()
    assert lib.hp_zones_reset(dom.h) == -5 and b"hp_zones_reset between hp_step_begin and hp_step_end" in lib.hp_last_error()
    desc = hp.ZonesDesc(C.sizeof(hp.ZonesDesc), 4, zone_count, 0, ids16.ctypes.data_as(C.POINTER(C.c_uint16)), FLOOD)
    assert lib.hp_zones_enable(dom.h, C.byref(desc)) == -5 and b"hp_zones_enable between hp_step_begin and hp_step_end" in lib.hp_last_error()
    assert raw_info(dom)[0] == before
    dom.step_end()
    goes_on()
    # a partial read, queued behind the samples: records [2, 5)
    stride = raw_info(dom)[2]
    assert lib.hp_zones_read(dom.h, 2, 3, out) == 0
    dom.sync()
    assert np.array_equal(buf[:3 * stride].reshape(3, stride), ref[0].words()[2:5])
    dom.zones_disable()
    dom.zones_disable()
    ref[0] = None
    fails(-5, "before hp_zones_enable", dom.zones_sample)
    dom.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_save_and_restore():
    cols, rows = 257, 130
    st, bed, man = syn.s_rough(cols, rows, seed=5)
    ids, zone_count = layout("blocks", cols, rows)
    batches = (6, 7, 8, 5)
    dom = hp.Domain(cols, rows, dx=DX)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.zones_enable(ids, zone_count, capacity=16)

    def advance(some):
        for n in some:
            dom.step_batch(n)
            dom.zones_sample()

    logs = []
    hp.set_log_sink(lambda level, text: logs.append((level, text)))
    try:
        advance(batches[:2])
        dom.state_save()
        advance(batches[2:])
        first, state = dom.zone_records(), dom.download()
        assert raw_info(dom)[0] == 4
        dom.state_restore()
        assert raw_info(dom)[0] == 2 and dom.zones_info()["samples"] == 2
        advance(batches[2:])
        assert np.array_equal(dom.download(), state)
        assert_words(dom.zone_records(), first)
        assert first.shape[0] == 4 and not logs
        # a reset between save and restore: count 0, exactly one warning
        dom.state_save()
        advance((3,))
        assert dom.lib.hp_zones_reset(dom.h) == 0
        advance((2,))
        assert raw_info(dom)[0] == 1
        dom.state_restore()
        assert raw_info(dom)[0] == 0
        warnings = [text for level, text in logs if level == 8]
        assert len(warnings) == 1 and "zone sample count" in warnings[0], logs
        advance((4,))                                                             # ... and the recorder records on
        assert raw_info(dom)[0] == 1
        # with the recorder off a restore says nothing
        dom.zones_disable()
        dom.state_restore()
        assert len([1 for level, _ in logs if level == 8]) == 1
    finally:
        hp.set_log_sink(None)
    dom.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_strips_gather_zones(world):
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", lib,
                               os.path.join(os.path.dirname(lib), "fake_rccl.cpp")])
    res = subprocess.run([sys.executable, os.path.join(HERE, "zones_strips_worker.py"), str(world)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "zones identical in every word True" in res.stdout and "every zone carries water True" in res.stdout


@pytest.mark.parametrize("world", [2, 3])
def test_strip_runner_gather_zones(world, tmp_path):
    """StripRunner.zones_enable / zones_sample / gather_zones themselves: process ranks (torch.distributed.run) on the one GPU
    over the rehearsal transport, against Domain.zones() of the single domain after the same batches and samples."""
    from test_gpu_output_stage import _torchrun
    cols, rows, zone_count = 257, 130, 13
    y, x = np.mgrid[0:rows, 0:cols]
    ids = 1 + (x * 3 // cols) + 3 * (y * 4 // rows)            # zones that straddle every cut, and cut where no strip border is
    ids[:40, :50] = np.random.default_rng(1).integers(0, 14, (40, 50))
    raster, out = os.path.join(str(tmp_path), "ids.npy"), os.path.join(str(tmp_path), "zones.npz")
    np.save(raster, ids)
    r = _torchrun(world, [os.path.join(HERE, "zones_rehearsal_worker.py"), out, raster, str(zone_count), repr(FLOOD), repr(DX)]
                  + [str(n) for n in BATCHES], timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = np.load(out)
    st, bed, man = syn.s_rough(cols, rows)
    single = hp.Domain(cols, rows, dx=DX)
    single.upload(st, bed, man)
    single.set_target_time(1e9)
    single.zones_enable(ids, zone_count, flood_depth=FLOOD)
    for n in BATCHES:
        single.step_batch(n)
        single.zones_sample()
    want = single.zones()
    single.close()
    assert len(want["t"]) == len(BATCHES) and (want["wet"] > 0).all() and (want["volume"] > 0).all()
    assert set(got.files) == set(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert np.array_equal(got[key].view(np.uint64), want[key].view(np.uint64)), key


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_model_writes_the_same_file_from_the_device_and_from_the_host(tmp_path):
    from hipims_mi.model import Model
    from model_dir import make_newcastle
    zone_raster = np.zeros((195, 342))
    zone_raster[:100, :171] = 1; zone_raster[:100, 171:] = 2; zone_raster[100:, :200] = 3     # the north-east corner is in no zone
    files = {}
    for tag, device in (("device", True), ("host", False)):
        xml = make_newcastle(tmp_path / tag, duration=600, frequency=60)
        text = open(xml).read()
        marker = '<dataSource type="raster" value="structure,dem" source="NewcastleCentreDEM_2m.img" />'
        assert marker in text
        open(xml, "w").write(text.replace(marker, marker + '\n<dataSource type="raster" value="zones" source="zones.npy"/>'))
        np.save(os.path.join(str(tmp_path / tag), "topography", "zones.npy"), zone_raster)
        m = Model(xml, output_format=".npy", device_outputs=device, zone_flood_depth=0.001, zone_capacity=5)
        m.scheme.automatic_queue = False                                      # (batch boundaries are not physics-neutral: fixed)
        m.scheme.queue_addition_size = 16
        assert m.device_zones is device and (m.host_zones is None) is device
        m.run(max_outputs=2)
        series, samples = m.zones(), m.scheme.iterations // 16
        m.close()
        files[tag] = open(os.path.join(str(tmp_path / tag), "output", "zones.csv"), "rb").read()
        assert series["t"].shape == (samples,) and samples > 5                # (the device buffer of 5 was drained on the way)
        assert files[tag].count(b"\n") == 1 + 3 * samples
        assert (series["wet"][-1] > 0).all() and (series["volume"][-1] > 0).all()
    assert files["device"] == files["host"]
    assert files["host"].startswith(b"time,zone,cells,wet_area,flooded_area,volume,max_depth,max_speed\n")
