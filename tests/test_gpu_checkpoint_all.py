"""hp_state_save / hp_state_restore with every store that takes part in a checkpoint switched on at once: the peak tracker, the probe
and the zone recorder, the moving bed, the links' records, the infiltration's F, the open boundary's records and the tracer's M
(csrc/hp_checkpoint.hpp: the mark; csrc/hp_domain.hpp: the slot; csrc/hp_actors.hpp: the table of participants).

One domain of 24 x 16 cells: a closed ring with rows 4..11 of its east edge opened again, a pool over the west columns, rain, one link
from the pool to the shallow side, one bed shape of three cells, two soil classes, one tracer source, two gauges and two zones.  The
library refuses a tracer on a domain with link groups or an infiltration, and either of them on a domain with a tracer
(hp_tracer_enable, hp_boundary_add_links, hp_boundary_add_infiltration: HP_ERR_UNSUPPORTED), so "every store" is two line-ups of the
same scene: SOIL -- peaks, probes, zones, bed, links, F, open -- and TRACER -- peaks, probes, zones, bed, open, M.  Every store is in
at least one of them, and every case below runs on both.

Nothing here is compared against a reference: a restore followed by the same calls must give the same bits as the first time."""
import numpy as np
import pytest

import hipims_mi as hp
from hipims_mi import synthetic as syn

pytestmark = pytest.mark.gpu
COLS, ROWS, DX = 24, 16, 2.0
REAL = dict(f64=np.float64, f32=np.float32)
RAIN = dict(definition=hp.UNIFORM_RAIN_INTENSITY, series=[(0.0, 20.0), (100.0, 20.0), (200.0, 20.0)], interval=100.0, length=200.0)
OPEN = [dict(edge="east", first=4, last=11)]
LINK = [dict(a=(4, 5), b=(19, 10), kind="orifice", level=0.3, size=1.0, coeff=0.6, limit=np.inf)]
SHAPE = dict(cells=[(12, 7), (12, 8), (13, 8)], target=[0.2, 0.25, 0.2], series=[(0.0, 0.0), (0.5, 1.0)])
SHAPE_CELLS = [y * COLS + x for x, y in SHAPE["cells"]]
CLASSES = [dict(ks=3.3e-5, suction=0.05, deficit=0.35, capacity=np.inf), dict(ks=1e-5, suction=0.1, deficit=0.3, capacity=0.001)]
SOURCE = dict(cells=[(6, 6)], series=[(0.0, 0.0), (0.25, 4.0), (5.0, 1.0)])
GAUGES = [(5, 5), (20, 9)]
PEAKS = ["peakspeed", "hazard"]
BATCHES = (1, 2, 1)                                      # the 4 iterations of every leg
LINEUPS = dict(soil=("peaks", "probes", "zones", "bed", "links", "soil", "open"), tracer=("peaks", "probes", "zones", "bed", "open", "tracer"))
# what a reading holds of each store, its warning when the checkpoint is not its own, and what it is left with then
KEYS = dict(peaks=("peaks", "peaks_info"), probes=("probes", "probe_samples"), zones=("zones", "zone_samples"), bed=("bed",), links=("links",),
            soil=("F",), open=("open",), tracer=("M", "tracer_iterations"))
WARNING = dict(peaks="holds no peaks", probes="probe sample count", zones="zone sample count", bed="bed shapes were added or cleared",
               links="link groups were added or cleared", soil="infiltration was added or cleared", open="open segments were added or cleared",
               tracer="tracer was enabled or disabled")
OUTCOME = dict(peaks="reset", probes="zeroed", zones="zeroed", bed="left", links="zeroed", soil="left", open="zeroed", tracer="left")


def scene(real):
    y, x = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    bed = syn.round4(1.0 - 0.03 * x + 0.05 * np.sin(y))
    st = np.zeros((ROWS, COLS, 4))
    st[..., 0] = bed + 0.1
    st[:, :11, 0] = 1.8
    st[..., 1] = st[..., 0]
    st[:, 18:, 2] = 0.2                                  # towards the open edge
    syn._walls(st, bed)
    bed[4:12, -1] = syn.round4(bed[4:12, -2] - 0.02)     # the opened part of the ring: a real bed, dry
    st[4:12, -1, :2] = bed[4:12, -1, None]
    return st.astype(real), bed.astype(real), np.full((ROWS, COLS), 0.03, real)


def soil_raster():
    soil = np.zeros((ROWS, COLS), np.uint8)
    soil[:, :12], soil[:, 12:] = 1, 2
    return soil


def zone_raster():
    ids = np.zeros((ROWS, COLS), np.uint16)
    ids[1:-1, 1:12], ids[1:-1, 12:-1] = 1, 2
    return ids


def blob():
    y, x = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    r2 = (x - 10.5) ** 2 + (y - 8.0) ** 2
    return np.where(r2 < 25.0, 2.0 * np.exp(-r2 / 12.0), 0.0)


ENABLE = dict(
    peaks=lambda d: d.peaks_enable(PEAKS),
    probes=lambda d: d.probes_enable(gauges=GAUGES),
    zones=lambda d: d.zones_enable(zone_raster(), zone_count=2),
    bed=lambda d: d.bed_shape_add(SHAPE["cells"], SHAPE["target"], SHAPE["series"]),
    links=lambda d: d.add_links(LINK),
    soil=lambda d: d.add_infiltration(soil_raster(), CLASSES, initial=np.full((ROWS, COLS), 0.03125)),
    open=lambda d: d.add_open(OPEN),
    tracer=lambda d: (d.tracer_enable(blob()), d.tracer_add_source(SOURCE["cells"], SOURCE["series"])),
)
# the call that bumps a store's epoch while the others keep theirs
STALE = dict(
    peaks=lambda d: (d.peaks_disable(), d.peaks_enable(PEAKS)),
    probes=lambda d: d.lib.hp_probes_reset(d.h),
    zones=lambda d: d.lib.hp_zones_reset(d.h),
    bed=lambda d: d.bed_shape_add([(5, 11)], [0.9], [(0.0, 0.0), (1.0, 1.0)]),
    links=lambda d: d.add_links([dict(a=(6, 3), b=(17, 3), kind="pump", level=0.0, size=0.1)]),
    soil=ENABLE["soil"],                                  # (hp_boundary_clear would bump the links' and the open boundary's too: the case saves without it)
    open=lambda d: d.add_open([dict(edge="south", first=3, last=6)]),
    tracer=lambda d: (d.tracer_disable(), d.tracer_enable(blob() + 0.03125)),
)


def make(precision, stores):
    st, bed, man = scene(REAL[precision])
    dom = hp.Domain(COLS, ROWS, dx=DX, precision=precision)
    dom.upload(st, bed, man)
    dom.set_target_time(1e9)
    dom.add_uniform(RAIN["definition"], RAIN["series"], RAIN["interval"], RAIN["length"])
    dom.on = []
    enable(dom, stores)
    return dom


def enable(dom, stores):
    for s in stores:
        ENABLE[s](dom)
        dom.on.append(s)


def advance(dom):
    """One leg: 4 iterations in batches of 1, 2 and 1; behind each batch the bed moves and the three observers take a sample."""
    for n in BATCHES:
        dom.step_batch(n)
        if "bed" in dom.on:
            dom.bed_apply()
        for s in ("peaks", "probes", "zones"):
            if s in dom.on:
                getattr(dom, s + "_sample")()


def reading(dom):
    """Everything a checkpoint brings back, by name."""
    r = dict(state=dom.download(), scalars={k: v for k, v in dom.read_scalars().items() if k not in ("cells_calculated", "iterations")})    # (the host's own counts run on)
    if "peaks" in dom.on:
        r.update(peaks=dom.peaks(), peaks_info=dom.peaks_info())
    if "probes" in dom.on:
        r.update(probes=dom.probes(), probe_samples=dom.probes_info()["samples"])
    if "zones" in dom.on:
        r.update(zones=dom.zone_records(), zone_samples=dom.zones_info()["samples"])
    if "bed" in dom.on:
        r.update(bed=dom.download(hp.ARRAY_BED).reshape(-1)[SHAPE_CELLS])
    if "links" in dom.on:
        r.update(links=dom.links_read())
    if "soil" in dom.on:
        r.update(F=dom.infiltration_read())
    if "open" in dom.on:
        r.update(open=dom.open_read())
    if "tracer" in dom.on:
        r.update(M=dom.tracer_read(), tracer_iterations=dom.tracer_info()["iterations"])
    return r


def same(a, b):
    """In every bit."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return type(a) is type(b) and a == b


def differing(a, b):
    return [k for k in a if not same(a[k], b.get(k))]


def zeroed(v):
    return (isinstance(v, np.ndarray) and not np.frombuffer(v.tobytes(), np.uint8).any()) or (not isinstance(v, (np.ndarray, dict)) and v == 0) or \
        (isinstance(v, dict) and all(a.size == 0 for a in v.values()))


class Warnings:
    def __enter__(self):
        self.lines = []
        hp.set_log_sink(lambda level, text: self.lines.append((level, text)))
        return self

    def __exit__(self, *exc):
        hp.set_log_sink(None)

    @property
    def texts(self):
        return [text for level, text in self.lines if level == 8]


def assert_stale_outcome(store, before, after, fresh_peaks):
    """The table of the stores' stale outcomes: reset, zeroed, or left as it is."""
    for key in KEYS[store]:
        if OUTCOME[store] == "left":
            assert same(after[key], before[key]), (store, key)
        elif OUTCOME[store] == "zeroed":
            assert zeroed(after[key]), (store, key, after[key])
        elif key == "peaks":
            assert same(after[key], fresh_peaks), (store, key)
        else:
            assert after[key]["samples"] == 0, (store, key, after[key])


# 1, 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("lineup", list(LINEUPS))
def test_a_restore_replays_every_store_in_every_bit(lineup, precision):
    dom = make(precision, LINEUPS[lineup])
    advance(dom)
    at_save = reading(dom)
    dom.state_save()
    with Warnings() as w:
        advance(dom)
        first = reading(dom)
        dom.state_restore()
        assert differing(reading(dom), at_save) == []
        advance(dom)
        again = reading(dom)
    print({k: (float(np.abs(v["volume"]).sum()), int(v["active"].sum())) for k, v in first.items() if k in ("links", "open")})
    assert differing(first, again) == [] and w.texts == []
    # ... and the leg that was rolled back moved every store
    assert set(differing(first, at_save)) == set(first), differing(first, at_save)
    assert first["peaks_info"]["samples"] == first["probe_samples"] == first["zone_samples"] == 6 and first["open"]["volume"].sum() > 0
    if lineup == "soil":
        assert first["links"]["volume"].sum() > 0 and (first["F"] > at_save["F"]).any()
    else:
        assert first["tracer_iterations"] == 8
    dom.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lineup,store", [(l, s) for l, stores in LINEUPS.items() for s in stores])
def test_a_store_changed_since_the_save_is_warned_about_once_and_the_others_come_back(lineup, store):
    saved_without = ("soil",) if store == "soil" else ()
    dom = make("f64", [s for s in LINEUPS[lineup] if s not in saved_without])
    advance(dom)
    at_save = reading(dom)
    dom.state_save()
    advance(dom)
    if saved_without:
        enable(dom, saved_without)
    else:
        STALE[store](dom)
    fresh_peaks = dom.peaks()
    before = reading(dom)
    with Warnings() as w:
        dom.state_restore()
        after = reading(dom)
    assert len(w.texts) == 1 and WARNING[store] in w.texts[0], w.lines
    assert_stale_outcome(store, before, after, fresh_peaks)
    others = [k for k in at_save if k not in KEYS[store]]
    assert [k for k in others if not same(after[k], at_save[k])] == [] and len(others) == len(at_save) - (0 if saved_without else len(KEYS[store]))
    advance(dom)                                          # ... and the domain runs on
    assert np.isfinite(dom.download()).all()
    dom.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lineup", list(LINEUPS))
def test_a_checkpoint_taken_with_every_store_off_is_none_of_theirs(lineup):
    dom = make("f64", ())
    advance(dom)
    at_save = reading(dom)
    dom.state_save()
    enable(dom, LINEUPS[lineup])
    fresh_peaks = dom.peaks()
    advance(dom)
    before = reading(dom)
    with Warnings() as w:
        dom.state_restore()
        after = reading(dom)
    assert len(w.texts) == len(LINEUPS[lineup]), w.lines
    for store in LINEUPS[lineup]:
        assert sum(WARNING[store] in t for t in w.texts) == 1, (store, w.lines)
        assert_stale_outcome(store, before, after, fresh_peaks)
    assert same(after["state"], at_save["state"]) and same(after["scalars"], at_save["scalars"])
    advance(dom)
    assert np.isfinite(dom.download()).all()
    dom.close()
