"""hp_checkpoint.hpp: the mark a store keeps of its share of a checkpoint, and what hp_state_save / hp_state_restore ask it, pinned
without a GPU.

tests/checkpoint_probe.cpp is compiled with plain g++ and fed event lines; it prints the mark and the event's answer after each.  The
values expected here were NOT printed by the header: they are written out by hand from the statements the eight stores' *_save_reserve,
*_save and *_restore families made before they shared it (each test names the statements it restates)."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "hipims-ocl_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
NOTHING, BRING_BACK, STALE = 0, 1, 2
NEW = dict(taken=0, epoch=0, count=0, room=0)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("checkpoint") / "checkpoint_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "checkpoint_probe.cpp")])

    def run(events):
        """The mark and the answer after each of `events`, from a fresh mark."""
        out = subprocess.run([str(exe)], input="".join(e + "\n" for e in events), capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(events)
        return [{k: int(v) for k, v in (w.split("=") for w in line.split())} for line in out]
    return run


def answers(probe, events):
    return [r["answer"] for r in probe(events)]


def test_the_header_needs_no_hip():
    text = open(os.path.join(CSRC, "hp_checkpoint.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in text.splitlines())
    assert "getenv" not in code and "#include <hip" not in code and "hip/" not in code and "hp_domain" not in code


def test_without_a_checkpoint_a_restore_has_nothing_to_do(probe):
    """`if (!B.saved_taken) return HP_OK;` -- whatever the store's epoch."""
    assert answers(probe, ["verdict 0", "verdict 5"]) == [NOTHING, NOTHING]
    assert probe(["verdict 0"])[0] == dict(NEW, answer=NOTHING)


def test_a_checkpoint_of_the_stores_own_epoch_comes_back(probe):
    """`B.saved_taken = true; B.saved_epoch = B.epoch;`, then `B.saved_epoch != B.epoch` is false: the copy is brought back."""
    got = probe(["take 3 0", "verdict 3"])
    assert got[0] == dict(taken=1, epoch=3, count=0, room=0, answer=-1) and got[1] == dict(got[0], answer=BRING_BACK)


def test_a_change_of_epoch_since_the_save_makes_it_stale(probe):
    """`if (L.saved_epoch != L.epoch) { log_line(HP_LOG_WARNING, ...` -- added, cleared, enabled, disabled or reset since; an epoch
    only ever counts up, but the question is `!=`."""
    assert answers(probe, ["take 3 0", "verdict 4", "verdict 9", "verdict 2", "verdict 3"]) == [-1, STALE, STALE, STALE, BRING_BACK]


def test_a_store_saved_while_off_and_enabled_since_is_stale(probe):
    """tracer_save while off: `R.saved_taken = true; R.saved_epoch = R.epoch;` and nothing copied; hp_tracer_enable: `++R.epoch`."""
    assert answers(probe, ["take 4 0", "verdict 5"]) == [-1, STALE]
    # ... and one that is still off has its epoch, and copies nothing (`if (R.on)`: the store's own affair)
    assert answers(probe, ["take 4 0", "verdict 4"]) == [-1, BRING_BACK]


def test_a_copy_that_grows_with_its_store(probe):
    """bed_save_reserve / open_save_reserve: `if (!O.cells || O.cells <= O.saved_room) return HP_OK;` ... `O.saved_room = O.cells;`"""
    got = probe(["needs_room 0", "needs_room 10", "needs_room 6", "needs_room 10", "needs_room 11", "needs_room 0"])
    assert [r["answer"] for r in got] == [0, 1, 0, 0, 1, 0]
    assert [r["room"] for r in got] == [0, 10, 10, 10, 11, 11]
    assert all(r["taken"] == 0 and r["epoch"] == 0 for r in got)          # room is no checkpoint


def test_a_copy_of_a_fixed_size_is_allocated_once(probe):
    """links_save_reserve: `if (!L.links || L.saved) return HP_OK;` then LINK_MAX records, the same request every time."""
    assert answers(probe, ["needs_room 0", "needs_room 4096", "needs_room 4096", "needs_room 0", "needs_room 4096"]) == [0, 1, 0, 0, 0]


def test_a_freed_copy_is_allocated_again_and_the_mark_stays(probe):
    """soil_clear: soil_destroy frees S.saved and `++S.epoch`; saved_taken and saved_epoch are not touched.  With the infiltration
    added again the next hp_state_save finds `!S.saved` and allocates."""
    got = probe(["needs_room 384", "take 1 0", "lost_room", "verdict 3", "needs_room 384"])
    assert got[2] == dict(taken=1, epoch=1, count=0, room=0, answer=-1)
    assert [r["answer"] for r in got] == [1, -1, -1, STALE, 1]


def test_a_store_that_keeps_no_mark_while_off(probe):
    """peaks_save: `d->peaks.saved_valid = false; if (!d->peaks.on) return HP_OK;`, log_save: `g.saved_valid = g.on;` -- and
    peaks_restore / log_restore: `saved_valid && saved_epoch == epoch`, else reset / count 0."""
    assert answers(probe, ["take 2 7", "verdict 2", "drop", "verdict 2", "verdict 3"]) == [-1, BRING_BACK, -1, NOTHING, NOTHING]
    assert answers(probe, ["drop", "verdict 0"]) == [-1, NOTHING]
    assert answers(probe, ["take 2 7", "drop", "take 2 9", "verdict 2"]) == [-1, -1, -1, BRING_BACK]


def test_the_count_comes_back_with_the_copy(probe):
    """`d->peaks.saved_samples = d->peaks.samples;`, `g.saved_samples = g.samples;`, `R.saved_iterations = R.iterations;` -- as of the
    last save."""
    got = probe(["take 2 7", "verdict 2", "take 2 12", "take 3 0"])
    assert [r["count"] for r in got] == [7, 7, 12, 0]


def test_the_mark_survives_a_reset_of_its_store(probe):
    """hp_bed_shapes_clear: bed_destroy frees the copy, then `BedShapes none; none.epoch = B.epoch + 1; none.saved_taken = B.saved_taken;
    none.saved_epoch = B.saved_epoch; B = none;` -- the checkpoint taken at epoch 2 is stale for the store at epoch 3."""
    got = probe(["needs_room 5", "take 2 0", "carry", "verdict 3", "needs_room 5"])
    assert got[2] == dict(taken=1, epoch=2, count=0, room=0, answer=-1)
    assert [r["answer"] for r in got] == [1, -1, -1, STALE, 1]
    # ... and a store that had no checkpoint has none afterwards
    assert answers(probe, ["needs_room 5", "carry", "verdict 1"]) == [1, -1, NOTHING]
