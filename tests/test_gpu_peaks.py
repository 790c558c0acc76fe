"""The peak tracker on the device (hp_peaks_*; csrc/hp_peaks.hpp: track_peaks) against its NumPy restatement
(frontend.PeakTracker) fed the downloaded state and the device's time at every sample -- bit for bit: every operation is a
correctly rounded one and the sample order is fixed, so there are no tolerances.  GPU only."""
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
NAMES = list(hp.PEAK_CODES)
BATCHES = (3, 4, 5, 2, 1, 8)               # batches of pairs and of single iterations
ND = frontend.NODATA


def tracked_run(cols, rows, precision, scheme=hp.SCHEME_GODUNOV, seed=7, arrival_depth=0.01):
    """S-ROUGH, six samples after BATCHES, the doctored state uploaded before the third.  -> (domain, host tracker)"""
    real = np.float64 if precision == "f64" else np.float32
    st, bed, man = syn.s_rough(cols, rows, seed=seed, dtype=real)
    dom = hp.Domain(cols, rows, scheme=scheme, precision=precision)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.peaks_enable(NAMES, arrival_depth=arrival_depth)
    ref = frontend.PeakTracker(rows, cols, arrival_depth, t=dom.read_scalars()["time"])
    for k, n in enumerate(BATCHES):
        dom.step_batch(n)
        if k == 2:
            st2, bed = doctor(dom.download(), bed)
            dom.upload(st2, bed, None)                  # (does not touch the peaks)
        dom.peaks_sample()
        ref.fold(dom.download(), bed, dom.read_scalars()["time"])
    return dom, ref


def assert_peaks(dom, ref):
    want = ref.rasters()
    rows, cols = dom.rows, dom.cols
    got = dom.peaks()
    assert list(got) == NAMES
    for name in NAMES:
        assert got[name].dtype == np.float64 and got[name].shape == (rows, cols)
        assert not np.isnan(got[name]).any(), name
        assert np.array_equal(got[name], want[name]), (name, cols, rows, int((got[name] != want[name]).sum()))
    got32 = dom.peaks(NAMES, dtype=np.float32)
    for name in NAMES:
        assert got32[name].dtype == np.float32 and np.array_equal(got32[name], want[name].astype(np.float32)), name
    row0, nrows = (rows // 3, rows - rows // 3 - 1)
    for dtype in (np.float64, np.float32):
        part = dom.peaks(NAMES[::-1], dtype=dtype, row0=row0, nrows=nrows)
        empty = dom.peaks(["hazard", "peakspeed"], dtype=dtype, row0=rows, nrows=0)
        assert empty["hazard"].shape == empty["peakspeed"].shape == (0, cols)
        for name in NAMES:
            assert np.array_equal(part[name], want[name][row0:row0 + nrows].astype(dtype)), (name, dtype)
    info = dom.peaks_info()
    assert info == ref.info() and info["samples"] == len(BATCHES), (info, ref.info())
    return got


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("size", [(67, 45), (64, 3), (257, 130), (1031, 517)])
def test_device_peaks_equal_the_host_tracker(size, precision):
    cols, rows = size
    dom, ref = tracked_run(cols, rows, precision, seed=400 + cols)
    got = assert_peaks(dom, ref)
    if rows > 3:
        for name in NAMES:                               # every branch is there: tracked cells and cells that never were
            nodata = got[name] == ND
            assert nodata.any() and not nodata.all(), name
        assert (got["wetduration"][got["wetduration"] != ND] > 0).any()
        assert ((got["arrivaltime"] != ND) <= (got["peakspeed"] != ND)).all()      # over the arrival depth => wet
    dom.close()


@pytest.mark.parametrize("scheme", [hp.SCHEME_MUSCL_HANCOCK, hp.SCHEME_INERTIAL])
def test_device_peaks_equal_the_host_tracker_other_schemes(scheme):
    dom, ref = tracked_run(67, 45, "f64", scheme=scheme, seed=11)
    assert_peaks(dom, ref)
    dom.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [hp.MATH_FAST, hp.MATH_STRICT])
def test_tracking_does_not_perturb_the_run(mode):
    cols, rows = 257, 130
    st, bed, man = syn.s_rough(cols, rows, seed=3)
    seen = []
    for tracked in (False, True):
        dom = hp.Domain(cols, rows, math_mode=mode)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        if tracked:
            dom.peaks_enable(NAMES)
        for _ in range(8):
            dom.step_batch(8)
            if tracked:
                dom.peaks_sample()
        ps = dom.pair_stats()
        seen.append((dom.download(), dom.read_scalars(), dom.launch_counts(), (ps["pairs"], ps["skipped_rows"], ps["still_rows"])))
        if tracked:
            assert dom.peaks_info()["samples"] == 8
        dom.close()
    plain, tracked = seen
    assert np.array_equal(plain[0], tracked[0])
    assert plain[1] == tracked[1] and plain[1]["iterations"] == 64
    assert plain[2] == tracked[2] and plain[3] == tracked[3], (plain[2:], tracked[2:])


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_peaks():
    cols, rows = 257, 130
    st, bed, man = syn.s_rough(cols, rows, seed=5)
    batches = (6, 7, 8, 5, 9)

    def start():
        dom = hp.Domain(cols, rows)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        return dom

    def advance(dom, some):
        for n in some:
            dom.step_batch(n)
            dom.peaks_sample()

    straight = start()
    straight.peaks_enable(NAMES)
    advance(straight, batches)
    want, want_info, want_state = straight.peaks(), straight.peaks_info(), straight.download()
    straight.close()

    dom = start()
    dom.peaks_enable(NAMES)
    advance(dom, batches[:3])
    dom.state_save()
    advance(dom, batches[3:])
    assert dom.peaks_info() == want_info
    dom.state_restore()
    assert dom.peaks_info()["samples"] == 3
    advance(dom, batches[3:])
    got = dom.peaks()
    assert dom.peaks_info() == want_info and np.array_equal(dom.download(), want_state)
    for name in NAMES:
        assert np.array_equal(got[name], want[name]), name
    dom.close()

    # a snapshot taken before the tracker was enabled holds no peaks: reset, one warning
    logs = []
    hp.set_log_sink(lambda level, text: logs.append((level, text)))
    try:
        dom = start()
        dom.step_batch(5)
        dom.state_save()
        t_saved = dom.read_scalars()["time"]
        dom.peaks_enable(NAMES)
        advance(dom, (4,))
        assert (dom.peaks()["peakspeed"] != ND).any()
        dom.state_restore()
        got, info = dom.peaks(), dom.peaks_info()
        assert all((got[name] == ND).all() for name in NAMES)
        assert info == dict(samples=0, t_first=t_saved, t_last=t_saved)
        warnings = [text for level, text in logs if level == 8]
        assert len(warnings) == 1 and "holds no peaks" in warnings[0], logs
        # ... and with tracking off again a restore says nothing
        dom.peaks_disable()
        dom.state_restore()
        assert len([1 for level, _ in logs if level == 8]) == 1
        dom.close()
    finally:
        hp.set_log_sink(None)


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_state_errors():
    st, bed, man = syn.s_rough(64, 32, seed=2)
    dom = hp.Domain(64, 32)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    for call in (dom.peaks_sample, dom.peaks_reset, dom.peaks_info, lambda: dom.peaks(["hazard"]), dom.peaks):
        with pytest.raises(hp.HipimsError, match=r"\(-5\).*before hp_peaks_enable"):
            call()
    dom.peaks_disable()                                                       # idempotent
    dom.peaks_enable(["hazard"])                                              # one value: one accumulator
    dom.step_batch(3)
    dom.peaks_sample()
    assert list(dom.peaks()) == ["hazard"]
    with pytest.raises(hp.HipimsError, match=r"\(-1\).*does not track"):
        dom.peaks(["peakspeed"])
    with pytest.raises(hp.HipimsError, match="out of bounds"):
        dom.peaks(["hazard"], row0=1, nrows=32)
    dom.step_begin()
    for call in (dom.peaks_sample, lambda: dom.peaks(["hazard"])):
        with pytest.raises(hp.HipimsError, match=r"\(-5\).*between hp_step_begin and hp_step_end"):
            call()
    dom.step_end()
    dom.peaks_sample()
    dom.peaks_disable()
    dom.peaks_disable()
    with pytest.raises(hp.HipimsError, match="before hp_peaks_enable"):
        dom.peaks_sample()
    dom.peaks_enable(["arrivaltime", "peakspeed"], arrival_depth=0.5)          # disable followed by enable works
    ref = frontend.PeakTracker(32, 64, 0.5, t=dom.read_scalars()["time"])
    dom.step_batch(4)
    dom.peaks_sample()
    ref.fold(dom.download(), bed, dom.read_scalars()["time"])
    got = dom.peaks()
    assert list(got) == ["peakspeed", "arrivaltime"]
    for name in got:
        assert np.array_equal(got[name], ref.rasters()[name]), name
    dom.peaks_reset()
    assert dom.peaks_info()["samples"] == 0 and (dom.peaks()["peakspeed"] == ND).all()
    with pytest.raises(hp.HipimsError, match="arrival_depth"):
        dom.peaks_enable(["hazard"], arrival_depth=1e-9)
    assert (dom.peaks()["peakspeed"] == ND).all()                             # a refused enable has left the tracker as it was
    dom.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_strips_gather_peaks():
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", lib,
                               os.path.join(os.path.dirname(lib), "fake_rccl.cpp")])
    res = subprocess.run([sys.executable, os.path.join(HERE, "peaks_strips_worker.py"), "2"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "peaks bit-identical True" in res.stdout and "info equal True" in res.stdout


def test_strip_runner_gather_peaks(tmp_path):
    """StripRunner.peaks_enable / peaks_sample / gather_peaks themselves: two process ranks (torch.distributed.run) on the one
    GPU over the rehearsal transport, against the single domain's peaks after the same batches and samples."""
    from test_gpu_output_stage import _torchrun
    cols, rows = 96, 70
    out = os.path.join(str(tmp_path), "peaks.npz")
    r = _torchrun(2, [os.path.join(HERE, "peaks_rehearsal_worker.py"), out, str(cols), str(rows)] + [str(n) for n in BATCHES], timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = np.load(out)
    st, bed, man = syn.s_rough(cols, rows, manning=None)
    single = hp.Domain(cols, rows)
    single.upload(st, bed, man)
    single.set_target_time(1e9)
    single.peaks_enable(NAMES, arrival_depth=0.02)
    for n in BATCHES:
        single.step_batch(n)
        single.peaks_sample()
    want, want32, info = single.peaks(), single.peaks(["hazard", "wetduration"], dtype=np.float32), single.peaks_info()
    single.close()
    assert list(got["info"]) == [info["samples"], info["t_first"], info["t_last"]] and info["samples"] == len(BATCHES)
    for name in NAMES:
        assert got["f64_" + name].dtype == np.float64 and got["f64_" + name].shape == (rows, cols)
        assert np.array_equal(got["f64_" + name], want[name]), name
        assert (want[name] != ND).any(), name
    for name in ("hazard", "wetduration"):
        assert got["f32_" + name].dtype == np.float32 and np.array_equal(got["f32_" + name], want32[name]), name


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_samples_behind_speculative_strict_batches(tmp_path):
    """Every speculative batch is re-run (HP_STRICT_SPEC_FORCE=1): a sample enters the library behind it, so the replay comes
    first and the sample sees the replayed state -- the same peaks as without speculation."""
    outs = {}
    for tag, env in (("forced", dict(HP_STRICT_SPECULATE="1", HP_STRICT_SPEC_FORCE="1")), ("plain", {})):
        clean = {k: v for k, v in os.environ.items() if k not in ("HP_STRICT_SPECULATE", "HP_STRICT_SPEC_FORCE")}
        out = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, os.path.join(HERE, "peaks_spec_worker.py"), out], capture_output=True, text=True, timeout=300,
                           env=dict(clean, **env))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        outs[tag] = (np.load(out), int(r.stdout.split("replays=")[1].split()[0]))
    assert outs["forced"][1] == 3 and outs["plain"][1] == 0
    for key in ["state", "info"] + NAMES:
        assert np.array_equal(outs["forced"][0][key], outs["plain"][0][key]), key
    assert (outs["plain"][0]["hazard"] != ND).any()


# Model ------------------------------------------------------------------------------------------------------------------
def test_model_tracks_on_the_device_and_leaves_the_run_alone(tmp_path):
    from hipims_mi.model import Model
    from model_dir import make_newcastle
    runs = {}
    for tag, peaks in (("plain", None), ("peaks", ["arrivaltime", "wetduration", "hazard"])):
        m = Model(make_newcastle(tmp_path / tag, duration=360, frequency=120), output_format=".npy", peaks=peaks, peak_arrival_depth=0.001)
        m.scheme.automatic_queue = False                                      # (batch boundaries are not physics-neutral: fixed)
        m.scheme.queue_addition_size = 64
        assert m.device_peaks is (peaks is not None) and m.host_peaks is None
        outs = m.run()
        info = m.sim.peaks_info() if peaks else None
        runs[tag] = (outs, m.sim.download(), m.sim.read_scalars(), info, m.scheme.iterations)
        m.close()
    plain, tracked = runs["plain"], runs["peaks"]
    assert np.array_equal(plain[1], tracked[1]) and plain[2] == tracked[2]
    assert tracked[3]["samples"] * 64 == tracked[4] and tracked[3]["t_last"] == tracked[2]["time"] == 360.0
    assert len(plain[0]) == len(tracked[0]) == 3
    for (t, a), (_, b) in zip(plain[0], tracked[0]):
        assert set(b) == set(a) | {"arrivaltime", "wetduration", "hazard"}
        assert all(np.array_equal(a[name], b[name]) for name in a)
        arrival, wet = b["arrivaltime"], b["wetduration"]
        assert np.array_equal(arrival == ND, wet == ND) and (arrival != ND).any() and (arrival == ND).any()
        assert (arrival[arrival != ND] <= t).all() and (wet[wet != ND] <= t).all() and (wet[wet != ND] >= 0).all()
