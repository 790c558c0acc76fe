"""The output stage on the device: Domain.derive / Domain.stats (hp_domain_derive / hp_domain_stats) against the host
derivation of the downloaded state (frontend.derive_output, the restatement of Datasets/CRasterDataset.cpp:185-267) --
bit for bit --, and NumPy for the statistics.  GPU only."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import hipims_mi as hp
from conftest import record
from hipims_mi import frontend, synthetic as syn
from test_gpu_edges import SIZES_3, SIZES_5

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["depth", "maxdepth", "fsl", "maxfsl", "dischargex", "dischargey", "velocityx", "velocityy", "froude"]
SIZES = sorted(set(SIZES_3 + SIZES_5)) + [(1024, 1024)]


def doctor(state, bed):
    """Cells that hit every branch of the derivations and of the statistics (flat ids spread over the grid; on the
    smallest grids later edits overwrite earlier ones)."""
    st, zb = state.copy(), bed.copy()
    real = st.dtype.type
    rows, cols = zb.shape
    zb[0, :] = zb[-1, :] = zb[:, 0] = zb[:, -1] = real(9999.9)            # a closed-edge wall on each edge
    fs, fb = st.reshape(-1, 4), zb.reshape(-1)
    n = fb.size
    eps = real(1e-8)
    edits = [
        (1.0, None, -9999.0, 0.0, 0.0),                                    # disabled
        (2.0, 2.0, 2.0, 0.1, 0.1),                                         # Z == zb (with discharge: divided by zero on the host)
        (2.0, 1.5, 1.5, 0.1, -0.1),                                        # Z < zb: negative depth
        (0.0, eps, eps, 1e-9, 0.0),                                        # Z - zb == 1e-8 (as the precision has it) ...
        (0.0, np.nextafter(eps, real(1)), eps, 1e-9, 0.0),                 # ... one ulp above
        (0.0, np.nextafter(eps, real(0)), eps, 1e-9, 0.0),                 # ... one ulp below
        (1.0, 1.0 + 1e-8, 1.0 + 1e-8, 0.0, 1e-9),                          # the same threshold through a rounded sum
        (3.0, 4.0, 4.0, 0.0, 0.0),                                         # wet, at rest
        (3.0, 4.0, 3.0 + 9999.0, 0.2, 0.0),                                # Zmax - zb >= 9999
        (3.0, 4.0, 3.0 + 20000.0, 0.0, 0.2),
        (1.0, 51.0, 51.0, 3000.0, 4000.0),                                 # the deepest and fastest cell ...
        (1.0, 51.0, 51.0, 3000.0, 4000.0),                                 # ... twice: ties go to the lowest id
        (9999.9, 10001.0, 10001.0, 1.0, 1.0),                              # water on a wall: fsl masks it, stats skip it
        (5.0, 5.5, 5.25, -0.3, 0.4),                                       # Zmax below Z
    ]
    for k, (b, z, zmax, qx, qy) in enumerate(edits):
        i = (k * 7919 + cols + 1) % n
        fb[i] = real(b)
        fs[i] = (real(b if z is None else z), real(zmax), real(qx), real(qy))
    return st, zb


def developed(cols, rows, precision, scheme=hp.SCHEME_GODUNOV, steps=40, seed=5, **kw):
    """S-ROUGH after `steps` iterations, doctored, uploaded again.  -> (domain, bed on the host)"""
    real = np.float64 if precision == "f64" else np.float32
    st, bed, man = syn.s_rough(cols, rows, seed=seed, dtype=real)
    dom = hp.Domain(cols, rows, scheme=scheme, precision=precision, **kw)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.step_batch(steps)
    st2, bed2 = doctor(dom.download(), bed)
    dom.upload(st2, bed2, None)
    return dom, bed2


def assert_derives(dom, bed, names=NAMES, dtype=np.float64, row0=0, nrows=None, res=1.0):
    got = dom.derive(names, dtype=dtype, row0=row0, nrows=nrows)
    state = dom.download(row0=row0, nrows=nrows)
    hi = row0 + state.shape[0]
    for name in names:
        want = frontend.derive_output(name, state, bed[row0:hi], res)
        if dtype == np.float32:
            want = want.astype(np.float32)
        assert got[name].dtype == dtype and got[name].shape == want.shape
        assert not np.isnan(got[name]).any(), name
        assert np.array_equal(got[name], want), (name, dom.cols, dom.rows, int((got[name] != want).sum()))
        assert np.array_equal(got[name] == frontend.NODATA, want == frontend.NODATA), name
    return got


def numpy_stats(state, bed, dx=1.0, first_id=0):
    z, zmax, qx, qy = (state[..., k].astype(np.float64).ravel() for k in range(4))
    zb = bed.astype(np.float64).ravel()
    counted = (zmax > -9999.0) & (zb <= 9999.0)
    depth = z - zb
    d = np.maximum(0.0, depth)
    wet = counted & (depth > 1e-8)
    with np.errstate(divide="ignore", invalid="ignore"):
        speed = np.where(wet, np.sqrt((qx / depth) ** 2 + (qy / depth) ** 2), -1.0)
    dmask = np.where(counted, d, -1.0)
    out = dict(cells=int(counted.sum()), cells_wet=int(wet.sum()), volume=math.fsum(d[counted]) * dx * dx,
               max_depth=0.0, max_speed=0.0, max_depth_cell=None, max_speed_cell=None)
    if counted.any():
        out["max_depth"], out["max_depth_cell"] = float(dmask.max()), int(dmask.argmax()) + first_id      # argmax: the first = lowest id
    if wet.any():
        out["max_speed"], out["max_speed_cell"] = float(speed.max()), int(speed.argmax()) + first_id
    return out


def assert_stats(got, want, tag):
    for k in ("cells", "cells_wet", "max_depth", "max_speed", "max_depth_cell", "max_speed_cell"):
        assert got[k] == want[k], (tag, k, got[k], want[k])
    n = want["cells"]
    err = abs(got["volume"] - want["volume"]) / want["volume"] if want["volume"] > 0 else abs(got["volume"])
    bound = (n - 1) * 2.0 ** -53            # summing n non-negative terms in ANY order: derived, not tuned
    print(f"{tag}: volume {got['volume']!r} vs fsum {want['volume']!r}, relative error {err:.3e}, bound {bound:.3e}")
    record("output_stage_volume_" + tag, relative_error=err, bound=bound, cells=n)
    assert err <= bound, (tag, err, bound)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_rasters_are_bit_identical_with_the_host_derivation(precision):
    for k, (cols, rows) in enumerate(SIZES):
        scheme = hp.SCHEME_MUSCL_HANCOCK if (cols, rows) in SIZES_5 and (cols, rows) not in SIZES_3 else hp.SCHEME_GODUNOV
        dom, bed = developed(cols, rows, precision, scheme=scheme, seed=200 + k)
        got = assert_derives(dom, bed)
        assert_derives(dom, bed, dtype=np.float32)
        if (cols, rows) == (1024, 1024):                                      # every branch really is there
            for name in NAMES:
                nodata = got[name] == frontend.NODATA
                assert (name.startswith("discharge") and not nodata.any()) or (nodata.any() and not nodata.all()), name
            assert np.array_equal(dom.derive("MaxDepth_final")["MaxDepth_final"], got["maxdepth"])     # substring codes
        dom.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_derive_reads_the_buffer_download_reads_and_changes_nothing(mode):
    """Batches of 1, 2, 3, 40, 41 iterations with iteration pairs on, a checkpoint and a roll-back: in a child process,
    because the pair switch is read from the environment."""
    res = subprocess.run([sys.executable, os.path.join(HERE, "output_stage_worker.py"), mode], capture_output=True, text=True,
                         timeout=600, env=dict(os.environ, HP_TWO_STEP="1"))
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "same state True" in res.stdout and "derive calls" in res.stdout


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_row_ranges():
    dom, bed = developed(187, 64, "f64")
    full = dom.derive(NAMES)
    for row0, nrows in ((0, 1), (0, 64), (5, 17), (63, 1), (31, 33), (10, None)):
        part = assert_derives(dom, bed, row0=row0, nrows=nrows)
        hi = 64 if nrows is None else row0 + nrows
        for name in NAMES:
            assert np.array_equal(part[name], full[name][row0:hi])
    for row0 in (0, 20, 64):
        empty = dom.derive(["depth", "froude"], row0=row0, nrows=0)
        assert empty["depth"].shape == (0, 187) and empty["froude"].shape == (0, 187)
        assert dom.stats(row0=row0, nrows=0)["cells"] == 0
    for row0, nrows in ((-1, 2), (0, 65), (64, 1), (65, 0), (3, -1)):
        with pytest.raises(hp.HipimsError, match="out of bounds"):
            dom.derive(["depth"], row0=row0, nrows=nrows)
        with pytest.raises(hp.HipimsError, match="out of bounds"):
            dom.stats(row0=row0, nrows=nrows)
    dom.step_batch(3)                                                         # the domain is still usable
    assert_derives(dom, bed)
    dom.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_statistics(precision):
    for k, (cols, rows) in enumerate(SIZES):
        dom, bed = developed(cols, rows, precision, seed=300 + k)
        state = dom.download()
        got, again = dom.stats(), dom.stats()
        assert got == again and np.float64(got["volume"]).tobytes() == np.float64(again["volume"]).tobytes()
        want = numpy_stats(state, bed)
        assert_stats(got, want, f"{precision}_{cols}x{rows}")
        if (cols, rows) == (1024, 1024):
            assert got["max_depth"] == 50.0 and got["max_speed"] == 100.0      # the doctored pair: a tie, lowest id reported
            ties = np.flatnonzero((state[..., 0].ravel() == 51.0) & (bed.ravel() == 1.0))
            assert len(ties) == 2 and got["max_depth_cell"] == ties[0] == got["max_speed_cell"]
        # row ranges add up to the whole
        cuts = sorted({0, rows // 3, (2 * rows) // 3, rows})
        parts = [dom.stats(row0=a, nrows=b - a) for a, b in zip(cuts, cuts[1:])]
        for a, b, p in zip(cuts, cuts[1:], parts):
            assert_stats(p, numpy_stats(state[a:b], bed[a:b], first_id=a * cols), f"{precision}_{cols}x{rows}_rows{a}_{b}")
        assert sum(p["cells"] for p in parts) == got["cells"] and sum(p["cells_wet"] for p in parts) == got["cells_wet"]
        assert max(p["max_depth"] for p in parts) == got["max_depth"] and max(p["max_speed"] for p in parts) == got["max_speed"]
        total = sum(p["volume"] for p in parts)
        assert abs(total - want["volume"]) <= (got["cells"] - 1) * 2.0 ** -53 * want["volume"]
        dom.close()


# 5, 8 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    dom, bed = developed(4096, 4096, "f64", steps=20)
    got = dom.derive(NAMES)                                                   # nine fp64 rasters: 1.2 GB, in ONE call
    state = dom.download()
    stats = dom.stats()
    dom.close()
    return got, state, bed, stats


def test_4096_all_nine_values_in_one_call(big):
    got, state, bed, stats = big
    for name in NAMES:
        assert np.array_equal(got[name], frontend.derive_output(name, state, bed, 1.0)), name
        assert not np.isnan(got[name]).any()
    assert_stats(stats, numpy_stats(state, bed), "f64_4096x4096")


def test_rasters_larger_than_the_scratch_cap_are_derived_in_blocks(big):
    got, state, bed, _ = big
    cap = 256 << 20
    header = open(os.path.join(os.path.dirname(HERE), "include", "hipims_mi.h")).read()
    assert "256 MiB" in header                                                # the documented cap is the one assumed here
    assert 9 * 8 * 4096 * 4096 > cap
    block = cap // (9 * 8 * 4096)                                             # rows per block
    seams = list(range(block, 4096, block))
    assert len(seams) >= 4
    for s in seams:                                                           # the rows either side of every seam
        for name in NAMES:
            want = frontend.derive_output(name, state[s - 1:s + 1], bed[s - 1:s + 1], 1.0)
            assert np.array_equal(got[name][s - 1:s + 1], want), (name, s)


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_model_writes_the_same_rasters_without_a_state_download(tmp_path):
    from hipims_mi.model import Model
    from model_dir import make_newcastle
    runs = {}
    for device_outputs in (True, False, None):
        xml = make_newcastle(tmp_path / str(device_outputs), duration=600, frequency=120)
        lines = []
        m = Model(xml, output_format=".npy", log=lines.append, device_outputs=device_outputs)
        m.scheme.automatic_queue = False                                      # (batch boundaries are not physics-neutral: fixed)
        m.scheme.queue_addition_size = 64
        calls = []
        plain = m.sim.download
        m.sim.download = lambda *a, **k: (calls.append(1), plain(*a, **k))[1]
        outs = m.run()
        runs[device_outputs] = (outs, len(calls), m.device_outputs, lines, m.domain_stats, str(tmp_path / str(device_outputs)))
        m.close()
    dev, host, default = runs[True], runs[False], runs[None]
    assert dev[2] is True and host[2] is False and default[2] is True         # the default is the device path
    assert dev[1] == 0 and default[1] == 0 and host[1] == len(host[0]) == 5
    for other in (host, default):
        assert [t for t, _ in dev[0]] == [t for t, _ in other[0]]
        for (_, a), (_, b) in zip(dev[0], other[0]):
            assert set(a) == set(b) == {"depth", "velocityx", "velocityy", "fsl", "maxdepth"}
            for name in a:
                assert a[name].dtype == b[name].dtype == np.float64 and np.array_equal(a[name], b[name]), name
    files = sorted(os.listdir(os.path.join(dev[5], "output")))
    assert len(files) == 25
    for f in files:
        assert open(os.path.join(dev[5], "output", f), "rb").read() == open(os.path.join(host[5], "output", f), "rb").read(), f
    # the log: the reference's line at the start, the domain's figures after every output time
    assert dev[3][0].startswith("Initial domain volume: ") and dev[3][0].endswith(" m3")
    assert sum("Domain volume: " in l and "wet cells" in l and "max depth" in l for l in dev[3]) == 5
    assert len(dev[4]) == 6 and dev[4][0][1]["volume"] == 0.0 and dev[4][-1][1]["volume"] > 0.0
    assert dev[4][-1][1] == host[4][-1][1]


# 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("scheme", [hp.SCHEME_GODUNOV, hp.SCHEME_MUSCL_HANCOCK])
def test_strips_gather_outputs_and_stats(world, scheme):
    lib = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
    if not os.path.exists(lib):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", lib,
                               os.path.join(os.path.dirname(lib), "fake_rccl.cpp")])
    res = subprocess.run([sys.executable, os.path.join(HERE, "output_strips_worker.py"), str(world), str(scheme)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "rasters bit-identical True" in res.stdout and "statistics equal True" in res.stdout


def _torchrun(nproc, script_args, timeout=600):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(port)] + script_args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("scheme", [hp.SCHEME_GODUNOV, hp.SCHEME_MUSCL_HANCOCK])
def test_strip_runner_gather_outputs_and_gather_stats(world, scheme, tmp_path):
    """StripRunner.gather_outputs / gather_stats themselves: process ranks (torch.distributed.run) on the one GPU over the
    rehearsal transport, against the single domain's derive / stats."""
    cols, rows, steps = 200, 211, 60
    out = os.path.join(str(tmp_path), "outputs.npz")
    r = _torchrun(world, [os.path.join(HERE, "output_rehearsal_worker.py"), out, str(scheme), str(cols), str(rows), str(steps)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = np.load(out)
    st, bed, man = syn.s_rough(cols, rows, manning=None)
    single = hp.Domain(cols, rows, scheme=scheme)
    single.upload(st, bed, man)
    single.set_target_time(1e9)
    single.step_batch(steps)
    want, want32, state = single.derive(NAMES), single.derive(["depth", "froude"], dtype=np.float32), single.download()
    stats = single.stats()
    single.close()
    for name in NAMES:
        assert got["f64_" + name].dtype == np.float64 and np.array_equal(got["f64_" + name], want[name]), name
    for name in ("depth", "froude"):
        assert got["f32_" + name].dtype == np.float32 and np.array_equal(got["f32_" + name], want32[name]), name
    gathered = {k: got["stats_" + k].item() for k in stats}
    gathered = {k: (None if k.endswith("_cell") and v == -1 else v) for k, v in gathered.items()}
    assert stats["cells_wet"] > 0
    for k in ("cells", "cells_wet", "max_depth", "max_speed", "max_depth_cell", "max_speed_cell"):
        assert gathered[k] == stats[k], (k, gathered[k], stats[k])
    assert_stats(gathered, numpy_stats(state, bed), f"strips{world}_scheme{scheme}")


# the library's own argument checks on a LIVE domain (the Python wrapper cannot produce most of them) ---------------------
def test_bad_arguments_on_a_live_domain_are_invalid_and_leave_it_usable():
    import ctypes as C
    dom, bed = developed(64, 32, "f64")
    lib, h = dom.lib, dom.h
    buf = np.zeros((32, 64))
    ok_values, ok_rasters = (C.c_int * 2)(hp.OUT_DEPTH, hp.OUT_FSL), (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    cases = [
        ((ok_values, 0, 8, ok_rasters, 0, 32), "count outside"),
        ((ok_values, hp.OUT_COUNT + 1, 8, ok_rasters, 0, 32), "count outside"),
        ((None, 2, 8, ok_rasters, 0, 32), "== NULL"),
        ((ok_values, 2, 8, None, 0, 32), "== NULL"),
        ((ok_values, 2, 2, ok_rasters, 0, 32), "element_bytes"),
        ((ok_values, 2, 16, ok_rasters, 0, 32), "element_bytes"),
        (((C.c_int * 2)(hp.OUT_DEPTH, hp.OUT_COUNT), 2, 8, ok_rasters, 0, 32), "unknown value 9"),
        (((C.c_int * 2)(-1, hp.OUT_FSL), 2, 8, ok_rasters, 0, 32), "unknown value -1"),
        (((C.c_int * 2)(hp.OUT_FSL, hp.OUT_FSL), 2, 8, ok_rasters, 0, 32), "listed twice"),
        ((ok_values, 2, 8, (C.c_void_p * 2)(buf.ctypes.data, None), 0, 32), "rasters[1] == NULL"),
        ((ok_values, 2, 8, ok_rasters, 1, 32), "out of bounds"),
        ((ok_values, 2, 8, ok_rasters, -1, 1), "out of bounds"),
    ]
    for args, message in cases:
        assert lib.hp_domain_derive(h, *args) == -1, message
        assert message.encode() in lib.hp_last_error(), (message, lib.hp_last_error())
    s = hp.DomainStats()
    assert lib.hp_domain_stats(h, 0, 32, C.byref(s)) == -1 and b"size mismatch" in lib.hp_last_error()      # struct_size 0
    assert lib.hp_domain_stats(h, 0, 32, None) == -1 and b"out == NULL" in lib.hp_last_error()
    s.struct_size = C.sizeof(hp.DomainStats)
    assert lib.hp_domain_stats(h, 0, 33, C.byref(s)) == -1 and b"out of bounds" in lib.hp_last_error()
    assert lib.hp_domain_stats(h, 0, 32, C.byref(s)) == 0 and s.cells > 0
    dom.step_batch(5)                                                         # none of it has hurt the domain
    assert_derives(dom, bed)
    dom.close()


# single-precision model files -------------------------------------------------------------------------------------------
def test_single_precision_model_keeps_the_host_path_by_default(tmp_path):
    """The front end keeps the bed in fp64 (4-decimal values, mostly not fp32 numbers) and its host derivation uses THAT bed
    with the fp32 state; the device holds the bed in fp32.  So for an fp32 domain the two paths are different functions of
    the bed, and the default stays the host path: the rasters a single-precision model file writes do not change.  The
    device path on request derives from the bed the domain holds."""
    from hipims_mi.model import Model
    from model_dir import make_newcastle
    runs = {}
    for device_outputs in (None, False, True):
        xml = make_newcastle(tmp_path / str(device_outputs), duration=360, frequency=120)
        text = open(xml).read().replace('value="double"', 'value="single"')
        assert 'value="single"' in text
        open(xml, "w").write(text)
        m = Model(xml, output_format=".npy", device_outputs=device_outputs)
        assert m.cfg.precision == "f32"
        m.scheme.automatic_queue = False
        m.scheme.queue_addition_size = 64
        outs = m.run()
        runs[device_outputs] = (outs, m.device_outputs, m.sim.download(), m.bed)
        m.close()
    default, host, dev = runs[None], runs[False], runs[True]
    assert default[1] is False and host[1] is False and dev[1] is True
    assert len(default[0]) == 3
    for (ta, a), (tb, b) in zip(default[0], host[0]):                          # the default writes what the host path writes
        assert ta == tb and all(np.array_equal(a[k], b[k]) for k in a)
    # the states are the same bits, so the device path's rasters are the host derivation over the fp32 bed
    assert np.array_equal(dev[2], host[2])
    bed32 = dev[3].astype(np.float32)
    for name, arr in dev[0][-1][1].items():
        assert arr.dtype == np.float64 and np.array_equal(arr, frontend.derive_output(name, dev[2], bed32, 2.0)), name
