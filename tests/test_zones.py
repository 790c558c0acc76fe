"""The zone recorder without a GPU: the NumPy restatement (frontend.ZoneRecorder, the reference the GPU tests hold the device
kernel to) against a plain Python loop over the cells, its independence of the partition (frontend.combine_zones), its consistency
with the statistics the output stage derives, the six hp_zones_* entry points and their descriptor, and the model file's `zones`
data source with the zones.csv it leads to.  Every word is an integer: the only tolerance is the derived bound of the volume."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

import hipims_mi as hp
import oracle
from hipims_mi import frontend
from model_dir import make_newcastle
from test_abi import HEADER, declared_functions

ZONE_FUNCTIONS = ["hp_zones_disable", "hp_zones_enable", "hp_zones_info", "hp_zones_read", "hp_zones_reset", "hp_zones_sample"]
KEYS = ("t", "cells", "wet", "flooded", "depth_hi", "depth_lo", "volume", "max_depth", "max_speed")


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def hand_made(cols, rows, seed, flood_depth):
    """A wet, moving random state with a wall ring, one disabled cell, one cell whose level lies below its bed, one of depth
    1000.5 m (the `hi` limb), one with NaN Qx and one of depth exactly flood_depth.  -> state, bed, the cells of those five."""
    rng = np.random.default_rng(seed)
    bed = rng.uniform(0.0, 2.0, (rows, cols))
    st = np.zeros((rows, cols, 4))
    st[..., 0] = bed + np.where(rng.random((rows, cols)) < 0.3, 0.0, rng.uniform(0.0, 1.5, (rows, cols)))
    st[..., 1] = st[..., 0]
    st[..., 2:] = rng.normal(0.0, 1.0, (rows, cols, 2))
    bed[0, :] = bed[-1, :] = bed[:, 0] = bed[:, -1] = 9999.9
    special = dict(disabled=(3, 2), below=(5, 4), deep=(7, 6), nan=(9, 8), threshold=(11, 10))
    x, y = special["disabled"]; st[y, x, 1] = -9999.0
    x, y = special["below"]; st[y, x, 0] = st[y, x, 1] = bed[y, x] - 0.25
    x, y = special["deep"]; bed[y, x] = 1.0; st[y, x, 0] = st[y, x, 1] = 1001.5
    x, y = special["nan"]; st[y, x, 0] = st[y, x, 1] = bed[y, x] + 0.75; st[y, x, 2] = np.nan
    x, y = special["threshold"]; bed[y, x] = 0.0; st[y, x, 0] = st[y, x, 1] = flood_depth
    return st, bed, special


def loop_record(st, bed, ids, zone_count, flood_depth, t):
    """One record in plain Python: floats for the arithmetic, unbounded ints for what is accumulated."""
    rows, cols = bed.shape
    words = [[0] * 7 for _ in range(zone_count + 1)]
    for y in range(rows):
        for x in range(cols):
            k = int(ids[y, x])
            z, zmax, qx, qy = (float(v) for v in st[y, x])
            zb = float(bed[y, x])
            if k == 0 or not (zmax > -9999.0 and zb <= 9999.0):
                continue
            depth = z - zb
            d = depth if depth > 0.0 else 0.0
            d = min(d, 1048576.0)
            q = int(round(d * 4294967296.0))          # (round() of a float: half to even)
            w = words[k]
            w[0] += 1
            w[1] += depth > 1e-8
            w[2] += depth > flood_depth
            w[3] += q >> 32
            w[4] += q & 0xffffffff
            w[5] = max(w[5], f64_bits(d))
            if depth > 1e-8:
                vx, vy = qx / depth, qy / depth
                sp = math.sqrt(vx * vx + vy * vy) if not (math.isnan(vx) or math.isnan(vy)) else math.nan
                if sp > 0.0:
                    w[6] = max(w[6], f64_bits(sp))
    return [f64_bits(t)] + [v for w in words[1:] for v in w]


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_zone_recorder_against_a_plain_loop():
    cols, rows, flood, dx = 23, 17, 0.1, 2.5
    st, bed, special = hand_made(cols, rows, 1, flood)
    rng = np.random.default_rng(2)
    ids = rng.integers(0, 5, (rows, cols))                                         # 0..4; zones 5 and 6 carried by no cell
    for name, k in (("disabled", 1), ("below", 2), ("deep", 3), ("nan", 4), ("threshold", 2)):
        ids[special[name][1], special[name][0]] = k
    rec = frontend.ZoneRecorder(ids, 6, flood, dx)
    rec.record(st, bed, 12.25)
    rec.record(st.astype(np.float32), bed.astype(np.float32), 13.5)                # an fp32 domain's values, widened
    got = rec.words()
    assert got.dtype == np.uint64 and got.shape == (2, 1 + 7 * 6)
    assert [int(v) for v in got[0]] == loop_record(st, bed, ids, 6, flood, 12.25)
    assert [int(v) for v in got[1]] == loop_record(st.astype(np.float32), bed.astype(np.float32), ids, 6, flood, 13.5)
    s = rec.series()
    assert sorted(s) == sorted(KEYS) and s["t"].tolist() == [12.25, 13.5]
    assert s["depth_hi"][0, 2] >= 1000 and s["max_depth"][0, 2] == 1000.5          # the deep cell: the `hi` limb (whole metres)
    assert (s["depth_hi"][0, [0, 1, 3]] < 1000).all()
    assert not got[:, 1 + 7 * 4:].any()                                            # zones no cell carries stay all-zero
    assert s["max_speed"][0, 3] > 0 and not np.isnan(s["max_speed"]).any()         # the NaN contributed nothing
    # depth == flood_depth is wet but not flooded; a level below the bed is counted, dry and adds no depth
    x, y = special["threshold"]
    alone = np.zeros((rows, cols), int); alone[y, x] = 1
    one = frontend.ZoneRecorder(alone, 1, flood, dx); one.record(st, bed, 0.0)
    assert one.words()[0, 1:4].tolist() == [1, 1, 0]
    x, y = special["below"]
    alone[:] = 0; alone[y, x] = 1
    one = frontend.ZoneRecorder(alone, 1, flood, dx); one.record(st, bed, 0.0)
    assert one.words()[0, 1:].tolist() == [1, 0, 0, 0, 0, 0, 0]
    # the volume: one rounding of the exact integer sum, then dx * dx
    S = (int(got[0, 1 + 7 * 2 + 3]) << 32) + int(got[0, 1 + 7 * 2 + 4])
    assert s["volume"][0, 2] == (S / 2 ** 32) * (dx * dx)
    with pytest.raises(ValueError):
        frontend.ZoneRecorder(ids, 3, flood, dx)                                   # an id above zone_count
    with pytest.raises(ValueError):
        frontend.ZoneRecorder(ids, 6, 1e-9, dx)
    with pytest.raises(ValueError):
        frontend.ZoneRecorder(ids, 4097, flood, dx)


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strips", [2, 3, 5])
def test_partition_invariance(strips):
    cols, rows, flood = 67, 45, 0.1
    st, bed, _ = hand_made(cols, rows, 10 + strips, flood)
    ids = np.random.default_rng(strips).integers(0, 8, (rows, cols))
    whole = frontend.ZoneRecorder(ids, 9, flood)
    cuts = [rows * k // strips for k in range(strips + 1)]
    parts = [frontend.ZoneRecorder(ids[a:b], 9, flood) for a, b in zip(cuts, cuts[1:])]
    for t in (1.0, 2.0):
        st[..., 0] += 0.01 * t
        whole.record(st, bed, t)
        for p, a, b in zip(parts, cuts, cuts[1:]):
            p.record(st[a:b], bed[a:b], t)
    combined = frontend.combine_zones([None] + [p.words() for p in parts])
    assert combined.dtype == np.uint64 and np.array_equal(combined, whole.words())
    assert whole.words()[:, 1:].any()
    parts[0].records[0][0] += np.uint64(1)
    with pytest.raises(RuntimeError, match="different model times"):
        frontend.combine_zones([p.words() for p in parts])


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_one_zone_over_everything_agrees_with_the_statistics():
    cols, rows, dx = 67, 45, 2.5
    st, bed, _ = hand_made(cols, rows, 3, 0.1)
    rec = frontend.ZoneRecorder(np.ones((rows, cols), int), 1, 0.1, dx)
    rec.record(st, bed, 0.0)
    s = rec.series()
    # domain_stats' derivation (csrc/hp_output.hpp), in NumPy
    z, zmax, qx, qy = (st[..., k].ravel() for k in range(4))
    zb = bed.ravel()
    counted = (zmax > -9999.0) & (zb <= 9999.0)
    depth = z - zb
    d = np.maximum(0.0, depth)
    wet = counted & (depth > 1e-8)
    with np.errstate(all="ignore"):
        speed = np.sqrt((qx / depth) * (qx / depth) + (qy / depth) * (qy / depth))
    cells = int(counted.sum())
    assert int(s["cells"][0, 0]) == cells and int(s["wet"][0, 0]) == int(wet.sum())
    assert s["max_depth"][0, 0] == d[counted].max() == 1000.5
    assert s["max_speed"][0, 0] == np.nanmax(speed[wet])
    volume = float(s["volume"][0, 0])
    for stats_volume in (dx * dx * math.fsum(d[counted]), dx * dx * float(np.sum(d[counted])), dx * dx * sum(d[counted].tolist())):
        # at most 2^-33 m per cell from the quantisation, plus the fp64 sum's own error bound: derived, not measured
        bound = cells * dx * dx * 2.0 ** -33 + cells * 2.0 ** -52 * volume
        print(f"volume {volume!r} vs {stats_volume!r}: difference {abs(volume - stats_volume):.3e}, bound {bound:.3e}")
        assert abs(volume - stats_volume) <= bound


# 4 ---------------------------------------------------------------------------------------------------------------------
def _with_zones(xml, source="zones.npy"):
    text = open(xml).read()
    marker = '<dataSource type="raster" value="structure,dem" source="NewcastleCentreDEM_2m.img" />'
    assert marker in text
    open(xml, "w").write(text.replace(marker, marker + f'\n<dataSource type="raster" value="zones" source="{source}"/>'))
    return xml


def _oracle_sim(cfg, cols, rows, res):
    return oracle.OracleSim(cols, rows, dx=res, scheme=cfg.scheme, very_small=cfg.dry_threshold, courant=cfg.courant,
                            end_time=cfg.duration, friction=cfg.friction, threads=4)


def newcastle_zones(rows=195, cols=342):
    ids = np.zeros((rows, cols))
    ids[:100, :171] = 1; ids[:100, 171:] = 2; ids[100:, :200] = 3                 # the north-east corner is in no zone
    return ids


def test_model_file_zones_and_the_csv(tmp_path):
    from hipims_mi.model import Model
    xml = _with_zones(make_newcastle(tmp_path / "z", duration=120, frequency=60))
    np.save(os.path.join(str(tmp_path / "z"), "topography", "zones.npy"), newcastle_zones())
    cfg = frontend.parse_configuration(xml)
    assert ("raster", ["zones"], "zones.npy") in cfg.sources
    plain = Model(make_newcastle(tmp_path / "plain", duration=120, frequency=60), make_sim=_oracle_sim, output_format=".npy")
    assert plain.zones() is None and plain.zone_ids is None
    m = Model(xml, make_sim=_oracle_sim, output_format=".npy", zone_flood_depth=0.001)
    assert np.array_equal(m.state0, plain.state0) and np.array_equal(m.bed, plain.bed)     # the data source changes nothing else
    assert m.host_zones is not None and not m.device_zones and m.zone_count == 3
    m.scheme.automatic_queue = False
    m.scheme.queue_addition_size = 8
    m.run(max_outputs=2)
    s, samples = m.zones(), m.scheme.iterations // 8
    assert s["t"].shape == (samples,) and samples >= 2 and s["cells"].shape == (samples, 3)
    # ... and what it records is the final state's record
    ref = frontend.ZoneRecorder(newcastle_zones(), 3, 0.001, m.res)
    ref.record(m.sim.download(), m.bed, m.scheme.current_time)
    assert np.array_equal(ref.words()[0], m.host_zones.words()[-1])
    assert (s["wet"][-1] > 0).all() and (s["volume"][-1] > 0).all()
    lines = open(os.path.join(str(tmp_path / "z"), "output", "zones.csv")).read().splitlines()
    assert lines[0] == "time,zone,cells,wet_area,flooded_area,volume,max_depth,max_speed"
    assert len(lines) == 1 + 3 * samples
    last = lines[-1].split(",")
    area = m.res * m.res
    assert last[:3] == [repr(float(s["t"][-1])), "3", str(int(s["cells"][-1, 2]))]
    assert [float(v) for v in last[3:]] == [int(s["wet"][-1, 2]) * area, int(s["flooded"][-1, 2]) * area, s["volume"][-1, 2],
                                            s["max_depth"][-1, 2], s["max_speed"][-1, 2]]
    m.close(); plain.close()
    # Model(zones=array) is the same thing
    m2 = Model(make_newcastle(tmp_path / "arr", duration=120, frequency=60), make_sim=_oracle_sim, output_format=None, zones=newcastle_zones())
    assert np.array_equal(m2.zone_ids, m.zone_ids) and m2.zone_ids.dtype == np.uint16
    m2.close()


@pytest.mark.parametrize("bad,message", [(1.5, "integers"), (-1.0, "0..4096"), (4097.0, "0..4096"), (np.nan, "integers")])
def test_model_rejects_a_bad_zone_raster(tmp_path, bad, message):
    from hipims_mi.model import Model
    xml = _with_zones(make_newcastle(tmp_path / "z", duration=120, frequency=60))
    ids = newcastle_zones()
    ids[7, 9] = bad
    np.save(os.path.join(str(tmp_path / "z"), "topography", "zones.npy"), ids)
    with pytest.raises(ValueError, match=message):
        Model(xml, make_sim=_oracle_sim, output_format=None)
    with pytest.raises(ValueError, match="cells, the domain"):
        Model(make_newcastle(tmp_path / "shape", duration=120, frequency=60), make_sim=_oracle_sim, output_format=None, zones=np.ones((10, 10)))


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_six_entry_points():
    lib = hp.load_library()
    assert [n for n in declared_functions() if n.startswith("hp_zones_")] == ZONE_FUNCTIONS
    for n in ZONE_FUNCTIONS:
        assert hasattr(lib, n) and n in hp.EXPORTS
    text = open(HEADER).read()
    assert "enum { HP_ZONE_WORDS = 7 }" in text and hp.ZONE_WORDS == 7
    # the descriptor: the header's fields in the header's order, at the offsets of the C layout (natural alignment)
    body = re.search(r"typedef struct \{([^}]*)\} hp_zones_desc_t;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t.replace(" ", ""), n) for t, n in re.findall(r"((?:const\s+)?\w+\s*\*?)\s*(\w+);", body)]
    ctype = {"uint32_t": C.c_uint32, "double": C.c_double, "constuint16_t*": C.POINTER(C.c_uint16)}
    assert [n for _, n in fields] == [n for n, _ in hp.ZonesDesc._fields_]
    offset = 0
    for (t, n), (_, py) in zip(fields, hp.ZonesDesc._fields_):
        assert py is ctype[t] or py == ctype[t], (n, t, py)
        size = C.sizeof(ctype[t])
        offset = -(-offset // size) * size
        assert getattr(hp.ZonesDesc, n).offset == offset and getattr(hp.ZonesDesc, n).size == size, n
        offset += size
    assert C.sizeof(hp.ZonesDesc) == -(-offset // 8) * 8 == 32


def test_argument_errors_come_before_any_device_use():
    lib = hp.load_library()

    def invalid(rc, message):
        assert rc == -1, (rc, message, lib.hp_last_error())
        assert message.encode() in lib.hp_last_error(), (message, lib.hp_last_error())

    ids = np.zeros(16, np.uint16)

    def desc(size=C.sizeof(hp.ZonesDesc), capacity=4, zones=2, raster=ids, flood=0.1):
        d = hp.ZonesDesc(size, capacity, zones, 0, raster.ctypes.data_as(C.POINTER(C.c_uint16)) if raster is not None else None, flood)
        return C.byref(d)

    invalid(lib.hp_zones_enable(None, None), "desc == NULL")
    invalid(lib.hp_zones_enable(None, desc(size=24)), "size mismatch")
    invalid(lib.hp_zones_enable(None, desc(capacity=0)), "capacity")
    invalid(lib.hp_zones_enable(None, desc(zones=0)), "zone_count outside 1..4096")
    invalid(lib.hp_zones_enable(None, desc(zones=4097)), "zone_count outside 1..4096")
    invalid(lib.hp_zones_enable(None, desc(raster=None)), "zone_of_cell == NULL")
    invalid(lib.hp_zones_enable(None, desc(flood=0.99e-8)), "flood_depth must be at least 1e-8")
    invalid(lib.hp_zones_enable(None, desc(flood=float("nan"))), "flood_depth must be at least 1e-8")
    invalid(lib.hp_zones_enable(None, desc(capacity=1171, zones=4096)), "256 MiB")       # 1171 x 28673 x 8 B is just over
    invalid(lib.hp_zones_enable(None, desc(capacity=1170, zones=4096)), "null domain")   # ... and 1170 just under
    invalid(lib.hp_zones_enable(None, desc()), "null domain")
    for f in (lib.hp_zones_disable, lib.hp_zones_reset, lib.hp_zones_sample):
        invalid(f(None), "null domain")
    n = C.c_uint64(0)
    invalid(lib.hp_zones_info(None, C.byref(n), C.byref(n), C.byref(n)), "null domain")
    buf = np.zeros(8, np.uint64)
    invalid(lib.hp_zones_read(None, 0, 1, buf.ctypes.data_as(C.POINTER(C.c_uint64))), "null domain")


# ---- strips over gloo: StripRunner.zones_enable / zones_sample / gather_zones themselves, on the oracle engine (no device path:
#      the ZoneRecorder fallback on every rank's downloaded strip) ---------------------------------------------------------------
STRIP_CASE = dict(cols=40, rows=36, batches=(7, 9, 4, 10), dx=2.5, flood=0.05, zone_count=12)


def strip_case_ids():
    """Zones that straddle every cut of worlds 2 and 3 (column blocks), zones cut along rows that are no strip borders, random
    ids (0 included) on one side, and a zone (12) that no cell carries."""
    c = STRIP_CASE
    y, x = np.mgrid[0:c["rows"], 0:c["cols"]]
    ids = 1 + (x * 2 // c["cols"]) + 2 * (y * 5 // c["rows"])           # bands change at rows 8, 15, 22, 29; cuts: 18, or 12 and 24
    ids[10:30, :9] = np.random.default_rng(3).integers(0, 12, (20, 9))
    return ids


def _strip_worker(rank, world, port, q):
    import functools
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from hipims_mi import strips, synthetic as syn
    from strip_oracle_engine import OracleStripEngine
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    c = STRIP_CASE
    st, bed, man = syn.s_rough(c["cols"], c["rows"], manning=None)
    r = strips.StripRunner(c["cols"], c["rows"], rank=rank, world=world,
                           engine_factory=functools.partial(OracleStripEngine, scheme=strips.SCHEME_GODUNOV))
    r.upload_global(st, bed, man)
    r.set_target_time(1e9)
    for call in (r.zones_sample, r.gather_zones):                       # before zones_enable: a message, not an AttributeError
        with pytest.raises(RuntimeError, match="zones_enable comes first"):
            call()
    r.zones_enable(strip_case_ids(), c["zone_count"], flood_depth=c["flood"], dx=c["dx"])
    assert r._zone_host is not None                                     # the oracle engine has no device path
    for n in c["batches"]:
        r.step(n)
        r.zones_sample()
    got = r.gather_zones()
    q.put((rank, got))
    r.close()


@pytest.mark.parametrize("world", [2, 3])
def test_strip_runner_gathers_zones_over_gloo(world):
    import torch.multiprocessing as mp
    from hipims_mi import strips, synthetic as syn
    from test_strips_gloo import _free_port
    c = STRIP_CASE
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_strip_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    answers = dict(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    got = answers[0]
    assert all(answers[r] is None for r in range(1, world))             # rank 0 alone receives the series
    st, bed, man = syn.s_rough(c["cols"], c["rows"], manning=None)
    single = oracle.OracleSim(c["cols"], c["rows"], quirks=oracle.QUIRKS_REFERENCE & ~oracle.Q6_MUSCL_SERIAL)
    single.upload(st, bed, man)
    single.set_target(1e9)
    ids = strip_case_ids()
    cuts = [p[1] for p in strips.partition(c["rows"], world, 1)[:-1]]
    assert all(len(set(ids[cut - 1]) & set(ids[cut])) >= 2 for cut in cuts)     # zones straddle every cut
    ref = frontend.ZoneRecorder(ids, c["zone_count"], c["flood"], c["dx"])
    for n in c["batches"]:
        single.run(n)
        ref.record(single.download(), bed, single.scalars()["t"])
    want = ref.series()
    assert want["t"][-1] > 0 and (want["wet"][-1, :11] > 0).all() and (want["max_speed"][-1, :11] > 0).all()
    assert not want["cells"][:, 11].any()
    assert set(got) == set(KEYS)
    for key in KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert np.array_equal(got[key].view(np.uint64), want[key].view(np.uint64)), key
