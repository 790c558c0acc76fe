"""hp_facts.hpp: what the engine knows about its buffers between launches, and the events that change it, pinned without a GPU.

tests/facts_probe.cpp is compiled with plain g++ and fed event names; it prints the facts after each.  The values expected here were
NOT printed by the header: they are written out by hand from the statements the entry points of hp_engine.hip made before the flags
moved -- each event from an all-set and from an all-clear start, the restore and the replay across a set and a clear copy, and the
findings of the last two reviews as the event sequences their host calls make."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "hipims-ocl_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))

FACTS = ("use_alt", "need_full_reduce", "edge_dirty", "rings_differ", "rings_checked", "other_stale", "m1_valid", "pair_fused_next",
         "still_rec_valid", "ghost_valid")
KEPT = ("saved.use_alt", "saved.need_full_reduce", "saved.edge_dirty", "saved.rings_differ", "saved.m1_valid", "saved.ghost_valid")

CUR_SET = dict(dict.fromkeys(FACTS, 1), ghost_valid=2)
CUR_CLEAR = dict.fromkeys(FACTS, 0)
SAVED_SET = dict(dict.fromkeys(KEPT, 1), **{"saved.ghost_valid": 2})
SAVED_CLEAR = dict.fromkeys(KEPT, 0)
NEW = dict(CUR_CLEAR, need_full_reduce=1, edge_dirty=1, **dict(SAVED_CLEAR, **{"saved.need_full_reduce": 1, "saved.edge_dirty": 1}))   # a domain as created

# how the four starts are reached (test_the_starts_are_what_they_are_called holds them to their names)
SET_CUR = ["rows_uploaded", "rings_compared 0", "pair_queued 1 1", "single_ended", "ghosts_exchanged 2"]
CLEAR_CUR = ["rows_uploaded", "full_state_uploaded 0", "edge_ring_priced", "maximum_priced", "time_control_changed", "pair_queued 0 0", "buffers_written_outside"]
STARTS = {
    "set": SET_CUR + ["checkpoint_taken", "pair_launched 1", "pair_ran 0 2"],
    "clear": ["edge_ring_priced", "maximum_priced", "checkpoint_taken"],
    "set, checkpoint clear": ["edge_ring_priced", "maximum_priced", "checkpoint_taken"] + SET_CUR + ["pair_launched 1", "pair_ran 0 2"],
    "clear, checkpoint set": SET_CUR + ["checkpoint_taken", "pair_launched 1", "pair_ran 0 2"] + CLEAR_CUR,
}
START_FACTS = {"set": dict(CUR_SET, **SAVED_SET), "clear": dict(CUR_CLEAR, **SAVED_CLEAR),
               "set, checkpoint clear": dict(CUR_SET, **SAVED_CLEAR), "clear, checkpoint set": dict(CUR_CLEAR, **SAVED_SET)}

# event -> what it changes from the all-set start, what it changes from the all-clear start
EVENTS = {
    "boundaries_or_bed_changed": ({"m1_valid": 0, "saved.m1_valid": 0}, {}),
    "time_control_changed": ({"m1_valid": 0}, {}),                                  # (the checkpoint's figure stays)
    "buffers_written_outside": ({"still_rec_valid": 0}, {}),
    "full_state_uploaded 4": ({"other_stale": 0, "rings_differ": 0, "use_alt": 0, "ghost_valid": 4},     # (rings_checked untouched)
                              {"need_full_reduce": 1, "edge_dirty": 1, "ghost_valid": 4}),
    "bed_uploaded": ({}, {"need_full_reduce": 1, "edge_dirty": 1}),
    "rows_uploaded": ({"rings_checked": 0}, {"need_full_reduce": 1, "edge_dirty": 1, "rings_differ": 1}),
    "rings_compared 1": ({"rings_differ": 0}, {"rings_checked": 1}),
    "rings_compared 0": ({}, {"rings_checked": 1}),
    "edge_ring_priced": ({"edge_dirty": 0}, {}),
    "maximum_priced": ({"need_full_reduce": 0}, {}),
    "single_begins": ({"m1_valid": 0}, {}),
    "other_made_current": ({"other_stale": 0}, {}),
    "single_ended": ({"use_alt": 0}, {"use_alt": 1}),
    "cold_started": ({}, {"m1_valid": 1}),
    "pair_queued 1 1": ({}, {"m1_valid": 1, "pair_fused_next": 1}),
    "pair_queued 1 0": ({"pair_fused_next": 0}, {"m1_valid": 1}),
    "pair_queued 0 1": ({"m1_valid": 0, "pair_fused_next": 0}, {}),
    "pair_queued 0 0": ({"m1_valid": 0, "pair_fused_next": 0}, {}),
    "pair_launched 1": ({}, {"still_rec_valid": 1}),
    "pair_launched 0": ({"still_rec_valid": 0}, {}),
    "pair_ran 0 4": ({}, {"other_stale": 1}),
    "pair_ran 1 4": ({"ghost_valid": 4}, {"other_stale": 1, "ghost_valid": 4}),
    "ghosts_consumed 1": ({"ghost_valid": 1}, {"ghost_valid": -1}),
    "ghosts_exchanged 4": ({"ghost_valid": 4}, {"ghost_valid": 4}),
    # use_alt, rings_differ, m1_valid and ghost_valid are the checkpoint's; need_full_reduce and edge_dirty are ORed with it
    "checkpoint_restored": ({"other_stale": 0, "rings_checked": 0, "pair_fused_next": 0}, {}),
    "spec_replayed": None,                                                           # (test_a_replay_...)
    "checkpoint_taken": None,                                                        # (test_a_checkpoint_keeps_six_facts)
    "spec_taken": None,
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("facts") / "facts_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "facts_probe.cpp")])

    def run(events):
        """The facts after the last of `events`, from a fresh BufferFacts."""
        out = subprocess.run([str(exe)], input="".join(e + "\n" for e in events), capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(events)
        return {k: int(v) for k, v in (w.split("=") for w in out[-1].split())}
    run.exe = str(exe)
    return run


def held(got, want):
    """`want` names every fact and every kept one; the predicates are checked where a test names them."""
    assert {k: got[k] for k in FACTS + KEPT} == {k: want[k] for k in FACTS + KEPT}


def test_the_header_needs_no_hip_and_reads_no_environment():
    text = open(os.path.join(CSRC, "hp_facts.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in text.splitlines())
    assert "getenv" not in code and "#include <hip" not in code and "hip/" not in code


def test_a_fact_is_not_assignable_from_outside(tmp_path):
    for stmt, ok in (("int v = f->use_alt; (void)v;", True), ("f->use_alt = 1;", False), ("f->m1_valid = false;", False), ("f.saved().m1_valid = false;", False)):
        src = tmp_path / "assign.cpp"
        src.write_text('#include "hp_facts.hpp"\nint main() { hp::BufferFacts f; %s return 0; }\n' % stmt)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True, text=True)
        assert (r.returncode == 0) == ok, (stmt, r.stderr[-2000:])


def test_every_event_of_the_header_is_in_the_table():
    text = open(os.path.join(CSRC, "hp_facts.hpp")).read()
    events = set(re.findall(r"^\tvoid (\w+)\(", text, re.M))
    assert events == {e.split()[0] for e in EVENTS}


def test_the_starts_are_what_they_are_called(probe):
    held(probe(["edge_ring_priced"]), dict(NEW, edge_dirty=0))
    for name, events in STARTS.items():
        held(probe(events), START_FACTS[name])
    got = probe(STARTS["clear"])
    assert (got["pair_ready.fixed"], got["pair_ready.dynamic"], got["strip_pair_ready.2"]) == (1, 1, 0)
    got = probe(STARTS["set"])
    assert (got["pair_ready.fixed"], got["pair_ready.dynamic"], got["strip_pair_ready.2"]) == (0, 0, 0)


@pytest.mark.parametrize("event", [e for e, v in EVENTS.items() if v is not None])
def test_event_from_all_set_and_from_all_clear(probe, event):
    for start, changes in zip(("set", "clear"), EVENTS[event]):
        held(probe(STARTS[start] + [event]), dict(START_FACTS[start], **changes))


def test_a_restore_takes_four_facts_from_the_checkpoint_and_keeps_the_marks_left_since(probe):
    held(probe(STARTS["set, checkpoint clear"] + ["checkpoint_restored"]),
         dict(START_FACTS["set, checkpoint clear"], use_alt=0, rings_differ=0, m1_valid=0, ghost_valid=0, other_stale=0, rings_checked=0, pair_fused_next=0))
    held(probe(STARTS["clear, checkpoint set"] + ["checkpoint_restored"]),
         dict(START_FACTS["clear, checkpoint set"], use_alt=1, rings_differ=1, m1_valid=1, ghost_valid=2, need_full_reduce=1, edge_dirty=1))


def test_a_checkpoint_keeps_six_facts(probe):
    held(probe(STARTS["set, checkpoint clear"] + ["other_made_current", "checkpoint_taken"]), dict(CUR_SET, other_stale=0, **SAVED_SET))
    held(probe(STARTS["clear, checkpoint set"] + ["checkpoint_taken"]), dict(CUR_CLEAR, **SAVED_CLEAR))


def test_a_replay_brings_back_fewer_facts_than_a_restore(probe):
    """use_alt, need_full_reduce, edge_dirty and ghost_valid; the checkpoint is not touched."""
    lower = ["single_ended", "edge_ring_priced", "maximum_priced", "ghosts_consumed 2", "rings_compared 1", "single_begins", "pair_queued 0 0"]
    before = dict(START_FACTS["set"], other_stale=0, use_alt=0, edge_dirty=0, need_full_reduce=0, ghost_valid=0, rings_differ=0, m1_valid=0, pair_fused_next=0)
    held(probe(STARTS["set"] + ["other_made_current", "spec_taken"] + lower), before)
    held(probe(STARTS["set"] + ["other_made_current", "spec_taken"] + lower + ["spec_replayed"]), dict(before, use_alt=1, edge_dirty=1, need_full_reduce=1, ghost_valid=2))
    held(probe(STARTS["clear"] + ["spec_taken"] + SET_CUR + ["pair_launched 1", "pair_ran 0 2", "spec_replayed"]),
         dict(CUR_SET, use_alt=0, edge_dirty=0, need_full_reduce=0, ghost_valid=0, **SAVED_CLEAR))


def test_the_predicates(probe):
    """pair_ready: use_alt == 0, the rings not in doubt, and with a dynamic timestep both remembered maxima good; strip_pair_ready: use_alt == 0
    and every ghost row valid."""
    p = lambda ev: (lambda g: (g["pair_ready.fixed"], g["pair_ready.dynamic"], g["strip_pair_ready.2"]))(probe(ev))
    assert p(["ghosts_exchanged 2"]) == (1, 0, 1)                                                       # a new domain: nothing priced yet
    assert p(["ghosts_exchanged 2", "edge_ring_priced"]) == (1, 0, 1)
    assert p(["ghosts_exchanged 2", "maximum_priced"]) == (1, 0, 1)
    assert p(["ghosts_exchanged 2", "edge_ring_priced", "maximum_priced"]) == (1, 1, 1)
    assert p(["ghosts_exchanged 2", "edge_ring_priced", "maximum_priced", "single_ended"]) == (0, 0, 0)
    assert p(["ghosts_exchanged 2", "edge_ring_priced", "maximum_priced", "ghosts_consumed 1"]) == (1, 1, 0)
    assert p(["edge_ring_priced", "maximum_priced", "rows_uploaded", "edge_ring_priced", "maximum_priced"]) == (0, 0, 0)   # the rings may differ
    assert p(["edge_ring_priced", "maximum_priced", "rows_uploaded", "edge_ring_priced", "maximum_priced", "rings_compared 0"]) == (0, 0, 0)
    assert p(["edge_ring_priced", "maximum_priced", "rows_uploaded", "edge_ring_priced", "maximum_priced", "rings_compared 1"]) == (1, 1, 0)


# ---- the findings of the last two reviews, as the events their host calls make ---------------------------------------------------------
UPLOAD = ["boundaries_or_bed_changed", "buffers_written_outside"]          # hp_domain_upload, before it looks at its arguments
UPLOAD_ROWS = ["time_control_changed", "buffers_written_outside", "rows_uploaded"]
BDY_PAIR = ["pair_queued 1 1", "pair_launched 0", "pair_ran 0 1"]
SPLIT_STEP = ["single_begins", "buffers_written_outside", "single_ended"]
SAVE = ["other_made_current", "checkpoint_taken"]                          # (repair_other_buffer first)
RESTORE = ["buffers_written_outside", "checkpoint_restored"]


def test_a_split_step_behind_a_boundary_pair_makes_the_next_pair_start_cold(probe):
    assert probe(BDY_PAIR)["m1_valid"] == 1 and probe(BDY_PAIR)["pair_fused_next"] == 1
    assert probe(BDY_PAIR + SPLIT_STEP)["m1_valid"] == 0
    assert probe(BDY_PAIR + SPLIT_STEP + ["cold_started"])["m1_valid"] == 1


def test_a_boundary_or_bed_change_inside_a_checkpoint_voids_its_m1_figure_and_a_new_time_does_not(probe):
    assert probe(BDY_PAIR + SAVE)["saved.m1_valid"] == 1
    assert probe(BDY_PAIR + SAVE + ["boundaries_or_bed_changed"] + RESTORE)["m1_valid"] == 0                 # hp_boundary_add_*
    got = probe(BDY_PAIR + ["edge_ring_priced", "maximum_priced"] + SAVE + UPLOAD + ["bed_uploaded"] + RESTORE)
    assert got["m1_valid"] == 0 and got["need_full_reduce"] == 1 and got["edge_dirty"] == 1                  # (the bed's own marks stay)
    assert probe(BDY_PAIR + SAVE + ["time_control_changed"])["m1_valid"] == 0                                # hp_set_time
    assert probe(BDY_PAIR + SAVE + ["time_control_changed"] + RESTORE)["m1_valid"] == 1
    assert probe(BDY_PAIR + SAVE + UPLOAD_ROWS + RESTORE)["m1_valid"] == 1                                   # (a partial upload spares it too)


def test_a_speculative_snapshot_is_taken_with_the_other_buffer_repaired(probe):
    pairs = ["pair_queued 0 1", "pair_launched 0", "pair_ran 0 1", "pair_queued 0 0", "pair_launched 0", "pair_ran 0 1"]
    assert probe(pairs)["other_stale"] == 1
    assert probe(pairs + ["buffers_written_outside", "other_made_current", "spec_taken"])["other_stale"] == 0
    r = subprocess.run([probe.exe], input="".join(e + "\n" for e in pairs + ["spec_taken"]), capture_output=True, text=True)
    assert r.returncode != 0 and "other_stale" in r.stderr, (r.returncode, r.stderr)       # the event's precondition
    r = subprocess.run([probe.exe], input="".join(e + "\n" for e in pairs + ["checkpoint_taken"]), capture_output=True, text=True)
    assert r.returncode != 0 and "other_stale" in r.stderr, (r.returncode, r.stderr)


def test_the_rings_are_compared_once_per_run_of_partial_uploads(probe):
    wanted = lambda g: g["rings_differ"] == 1 and g["rings_checked"] == 0                  # run_iterations: rings_really_differ is due
    assert wanted(probe(UPLOAD_ROWS + UPLOAD_ROWS))
    got = probe(UPLOAD_ROWS + UPLOAD_ROWS + ["rings_compared 1"])
    assert got["rings_differ"] == 0 and not wanted(got)
    got = probe(UPLOAD_ROWS + UPLOAD_ROWS + ["rings_compared 0"])
    assert got["rings_differ"] == 1 and not wanted(got)
    assert wanted(probe(UPLOAD_ROWS + ["rings_compared 1"] + UPLOAD_ROWS))


def test_a_restore_brings_the_rings_doubt_back_and_has_them_compared_anew(probe):
    seq = UPLOAD_ROWS + ["rings_compared 0"] + SAVE + UPLOAD + ["full_state_uploaded 1"]
    got = probe(seq)
    assert got["rings_differ"] == 0 and got["rings_checked"] == 1                          # (a full upload leaves rings_checked alone)
    got = probe(seq + RESTORE)
    assert got["rings_differ"] == 1 and got["rings_checked"] == 0


def test_a_device_pointer_to_the_state_voids_the_still_records_and_one_to_manning_does_not(probe):
    recorded = ["pair_queued 0 1", "pair_launched 1", "pair_ran 0 1"]
    assert probe(recorded)["still_rec_valid"] == 1                                         # hp_device_ptr(HP_PTR_MANNING) says nothing
    assert probe(recorded + ["buffers_written_outside"])["still_rec_valid"] == 0           # HP_PTR_STATE_NEXT_SRC / _OTHER / HP_PTR_BED
