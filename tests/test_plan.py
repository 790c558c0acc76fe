"""hp_plan.hpp: the host-side rules that decide what the next launch is, pinned without a GPU.

tests/plan_probe.cpp is compiled with plain g++ and fed one decision request per line; it prints every rule's answer.  The values
expected here were NOT printed by the header.  They come from two sources: rows written out by hand from the statements hp_engine.hip
made before the rules moved, and a Python transcription of each of those expressions (next to the line of hp_engine.hip at commit
4a7cf34 it was copied from), held against the probe over the full cross product of the rule's inputs -- or, where that exceeds
100 000 rows, a seeded sample of 100 000 of them."""
import itertools
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "hipims-ocl_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
GODUNOV, MUSCL, INERTIAL = 0, 1, 2
FAST, STRICT = 0, 1
AUTO, BASIC = 0, 1
Q1, QUIRKS = 1, 7
TAIL_MAX_BLOCKS = 65536

# what plan_probe.cpp takes for a field that a request does not name: a created domain under an empty environment
DEFAULTS = {
    "k.two_step": -1, "k.launch_tail": 1, "k.strip_reduce_always": 0, "k.pair_bdy": 1, "k.pair_strict": 1, "k.pair_exact": -1, "k.pair_skip": 1,
    "k.fill_after_pairs": 1, "k.strict_speculate": 0, "k.pair_tune": 1, "k.sweep_alternate": -1, "k.tail_max_blocks": TAIL_MAX_BLOCKS,
    "k.tail_max_blocks_k2k6": TAIL_MAX_BLOCKS, "k.march2_rseg_forced": 0, "k.fuse_bdy": 1,
    "scheme": GODUNOV, "kernel": AUTO, "math_mode": FAST, "precision": 8, "dynamic_dt": 1, "quirks": QUIRKS, "rows": 64, "cols": 96, "row_offset": 0,
    "ghost_rows": 1, "has_bdy": 0, "fusable": 0, "bdy_on_ring": 0, "bdy_removes_water": 0, "has_comm": 0, "comm_world": 1, "peer_direct": 0,
    "peer_mine": 0, "has_tail_words": 1, "tail_allowed": 0, "halo_overlap": 0, "split_now": 1, "strip_any_bdy": 0, "strip_first": 0,
    "strip_any_full": 0, "spec_now": 0, "has_stamps": 0, "march2_pays": 0, "has_links": 0, "soil_on": 0, "spec_fused_kept": 0,
    "f.use_alt": 0, "f.need_full_reduce": 1, "f.edge_dirty": 1, "f.rings_differ": 0, "f.other_stale": 0,
    "a.n": 8, "a.march2_rseg": 24, "a.tile_rows": 24, "a.blocks": 100, "a.first_of_batch": 0, "a.strip": 0, "a.exact": 0, "a.tail_want": 1,
    "a.part_all": 1, "a.own_stream": 1, "a.push_now": 0,
}


def complete(req):
    r = dict(DEFAULTS, **req)
    r.setdefault("cells", r["rows"] * r["cols"])
    r.setdefault("global_rows", r["rows"])
    return r


# ---- (b) the expressions of hp_engine.hip at 4a7cf34, transcribed ----------------------------------------------------------------------
def old_tail_limit(r):                                      # :49-53
    v = r["k.tail_max_blocks"]
    return v if v < TAIL_MAX_BLOCKS else TAIL_MAX_BLOCKS


def old_tail_limit_k2k6(r):                                 # :229-233
    return min(old_tail_limit(r), r["k.tail_max_blocks_k2k6"])


def old_make_tail_kind(r, limit):                           # :194, :207-220
    if not (r["a.tail_want"] and r["a.part_all"] and r["a.own_stream"] and r["a.blocks"] <= limit):
        return 0
    return 2 if r["a.push_now"] else 1


def old_sweep_alternates(r):                                # :245-250
    if r["k.sweep_alternate"] >= 0:
        return r["k.sweep_alternate"] != 0
    return r["precision"] == 4 or r["scheme"] == MUSCL


def old_pairs_possible_common(r):                           # :597-620
    mode = r["k.two_step"]
    if mode == 0 or (mode < 0 and not r["march2_pays"]):                                                        # :600
        return False
    bdy_size_ok = r["precision"] == 8 or r["cells"] >= 30000000 or mode > 0                                     # :609
    bdy_ok = (not r["has_bdy"]) or (r["k.pair_bdy"] and bdy_size_ok and r["fusable"] and not r["has_comm"] and r["comm_world"] <= 1
                                    and r["dynamic_dt"])                                                        # :610
    math_ok = r["math_mode"] == FAST or (r["k.pair_strict"] and not r["has_bdy"] and not r["has_comm"] and r["comm_world"] <= 1
                                         and r["dynamic_dt"] and not r["spec_now"])                             # :615-616
    return bool(r["scheme"] == GODUNOV and r["kernel"] != BASIC and math_ok and bdy_ok and (not r["dynamic_dt"] or (r["quirks"] & Q1) != 0)
                and r["k.launch_tail"] and r["has_tail_words"] and r["rows"] >= 5 and r["cols"] >= 5)           # :617-619


def old_pairs_possible(r):                                  # :621-625
    return bool(old_pairs_possible_common(r) and not r["has_comm"] and r["comm_world"] <= 1 and not r["peer_mine"] and r["row_offset"] == 0
                and r["global_rows"] == r["rows"])


def old_pair_ready(r):                                      # hp_facts.hpp: pair_ready
    return r["f.use_alt"] == 0 and not r["f.rings_differ"] and (not r["dynamic_dt"] or (not r["f.need_full_reduce"] and not r["f.edge_dirty"]))


def old_pair_eligible(r):                                   # :648-651
    return bool(old_pairs_possible(r) and old_pair_ready(r))


def old_strip_pairs_possible_here(r):                       # :655-658
    return bool(old_pairs_possible_common(r) and r["has_comm"] and r["comm_world"] > 1 and r["peer_direct"] and r["ghost_rows"] == 2
                and not r["f.rings_differ"])


def old_pair_exact(r):                                      # :663-671
    if r["math_mode"] == STRICT:
        return True
    if r["k.pair_exact"] >= 0:
        return r["k.pair_exact"] != 0
    return bool(r["bdy_removes_water"])                                                                         # (the loop over d->bdy, :668-669)


def old_pair_tile_rows(r):                                  # :733
    return min(r["a.march2_rseg"], 12) if (r["math_mode"] == STRICT and not r["k.march2_rseg_forced"]) else r["a.march2_rseg"]


def old_pair_records(r):                                    # :767
    return bool(r["precision"] == 8 and r["k.pair_skip"] and not r["a.strip"] and not r["has_bdy"] and not r["a.exact"]
                and r["math_mode"] != STRICT and r["a.tile_rows"] <= 32)


def old_fill_wanted(r):                                     # :863-865
    return bool(r["k.fill_after_pairs"] and r["f.other_stale"] and r["scheme"] == GODUNOV and r["kernel"] != BASIC
                and not (old_pair_exact(r) and r["has_stamps"]))


def old_spec_wanted(r):                                     # :1363-1385
    fusable_ok = True if r["spec_fused_kept"] else not r["fusable"]                                             # :1376-1380
    return bool(r["k.strict_speculate"] and r["a.n"] >= 8 and r["math_mode"] == STRICT and r["precision"] == 8 and not r["has_comm"] and fusable_ok
                and not r["has_links"] and not r["soil_on"] and r["kernel"] != BASIC and r["scheme"] in (GODUNOV, MUSCL))   # :1383-1384


def old_tuner_on(r):                                        # :1413-1417
    return bool(r["k.pair_tune"] and r["math_mode"] == STRICT and r["k.two_step"] != 1)


def old_everyone_step_begin(r):                             # :465-466, with d->strip_first
    q1, muscl = (r["quirks"] & Q1) != 0, r["scheme"] == MUSCL
    basic = r["kernel"] == BASIC and r["scheme"] == GODUNOV
    return bool(r["dynamic_dt"] and (muscl or not q1 or r["f.use_alt"] == 1 or basic or r["strip_any_bdy"] or (r["strip_first"] and r["strip_any_full"])))


def old_everyone_allreduce(r):                              # :1738-1745, with first_of_batch; None: strip_allreduce_max returned before the rule
    if not r["dynamic_dt"]:                                                                                     # :1738
        return None
    q1, muscl = (r["quirks"] & Q1) != 0, r["scheme"] == MUSCL
    basic = r["kernel"] == BASIC and r["scheme"] == GODUNOV
    return bool(muscl or not q1 or r["f.use_alt"] == 1 or basic or r["strip_any_bdy"] or (r["a.first_of_batch"] and r["strip_any_full"]))


def old_step_begin(r):                                      # step_begin_impl :410-474, launch_flux :374-399, :496-505
    has_bdy = r["has_bdy"] and r["scheme"] != MUSCL                                                             # :410
    q1, muscl = (r["quirks"] & Q1) != 0, r["scheme"] == MUSCL
    basic = r["kernel"] == BASIC and r["scheme"] == GODUNOV
    dst_is_primary = r["f.use_alt"] == 1
    cfl_mode, reprice = 0, False
    if r["dynamic_dt"] and not basic:                                                                           # :423
        if muscl or not q1 or dst_is_primary:
            cfl_mode = 1
        elif has_bdy:
            cfl_mode = 2
        else:
            cfl_mode = 0
        reprice = cfl_mode != 0 and (r["f.edge_dirty"] or (has_bdy and r["bdy_on_ring"]))                       # :431
    reduce_after = r["dynamic_dt"] and cfl_mode == 0 and (basic or r["f.need_full_reduce"])                     # :457 (and :500)
    priced = 1 if (r["dynamic_dt"] and cfl_mode != 0) else 0
    strips_ok = (not (r["has_comm"] and r["k.strip_reduce_always"])) if r["comm_world"] <= 1 else r["peer_direct"]   # :462
    fresh = priced
    if r["comm_world"] > 1 and r["peer_direct"]:
        everyone = old_everyone_step_begin(r)
        strips_ok = (priced != 0) == everyone
        fresh = 7 if everyone else 4
    tail_want = (r["k.launch_tail"] and r["tail_allowed"] and not basic and not reduce_after and strips_ok
                 and not (r["halo_overlap"] and r["split_now"]) and r["has_tail_words"])                        # :470-471
    edge_buffer = (r["f.use_alt"] ^ 1) if cfl_mode == 1 else r["f.use_alt"] if cfl_mode == 2 else 0             # :374-399
    return {"boundaries_applied": int(bool(has_bdy)), "cfl_mode": cfl_mode, "reprice_ring": int(bool(reprice)), "reduce_after": int(bool(reduce_after)),
            "tail_want": int(bool(tail_want)), "tail_fresh": fresh, "edge_buffer": edge_buffer, "reduce_buffer_is_primary": int(q1)}   # :501


BOOLS = (0, 1)
COMMON = {"k.two_step": (-1, 0, 1), "march2_pays": BOOLS, "k.launch_tail": BOOLS, "k.pair_bdy": BOOLS, "precision": (8, 4),
          "cells": (29999999, 30000000), "has_bdy": BOOLS, "fusable": BOOLS, "has_comm": BOOLS, "comm_world": (1, 2), "dynamic_dt": BOOLS,
          "k.pair_strict": BOOLS, "math_mode": (FAST, STRICT), "spec_now": BOOLS, "scheme": (GODUNOV, MUSCL, INERTIAL), "kernel": (AUTO, BASIC),
          "quirks": (QUIRKS, QUIRKS & ~Q1), "has_tail_words": BOOLS, "rows": (4, 5), "cols": (4, 5)}
# rule -> (its inputs and their values, what the parent computed: request -> {probe field: value})
RULES = {
    "pairs_possible_common": (COMMON, lambda r: {"pairs_possible_common": int(old_pairs_possible_common(r))}),
    "pairs_possible": (dict(COMMON, peer_mine=BOOLS, row_offset=(0, 2), global_rows=(4, 5, 9)), lambda r: {"pairs_possible": int(old_pairs_possible(r))}),
    "strip_pairs_possible_here": (dict(COMMON, peer_direct=BOOLS, ghost_rows=(1, 2, 4), **{"f.rings_differ": BOOLS}),
                                  lambda r: {"strip_pairs_possible_here": int(old_strip_pairs_possible_here(r))}),
    "pair_eligible": (dict(COMMON, peer_mine=BOOLS, row_offset=(0, 2), global_rows=(4, 5, 9),
                           **{"f.use_alt": BOOLS, "f.rings_differ": BOOLS, "f.need_full_reduce": BOOLS, "f.edge_dirty": BOOLS}),
                      lambda r: {"pair_eligible": int(old_pair_eligible(r))}),
    "pair_exact": ({"math_mode": (FAST, STRICT), "k.pair_exact": (-1, 0, 1), "bdy_removes_water": BOOLS}, lambda r: {"pair_exact": int(old_pair_exact(r))}),
    "pair_tile_rows": ({"math_mode": (FAST, STRICT), "k.march2_rseg_forced": BOOLS, "a.march2_rseg": (8, 12, 13, 24)},
                       lambda r: {"pair_tile_rows": old_pair_tile_rows(r)}),
    "pair_records": ({"precision": (8, 4), "k.pair_skip": BOOLS, "a.strip": BOOLS, "has_bdy": BOOLS, "a.exact": BOOLS, "math_mode": (FAST, STRICT),
                      "a.tile_rows": (12, 32, 33)}, lambda r: {"pair_records": int(old_pair_records(r))}),
    "fill_wanted": ({"k.fill_after_pairs": BOOLS, "f.other_stale": BOOLS, "scheme": (GODUNOV, MUSCL, INERTIAL), "kernel": (AUTO, BASIC),
                     "math_mode": (FAST, STRICT), "k.pair_exact": (-1, 0, 1), "bdy_removes_water": BOOLS, "has_stamps": BOOLS},
                    lambda r: {"fill_wanted": int(old_fill_wanted(r))}),
    "spec_wanted": ({"k.strict_speculate": BOOLS, "a.n": (7, 8), "math_mode": (FAST, STRICT), "precision": (8, 4), "has_comm": BOOLS, "fusable": BOOLS,
                     "spec_fused_kept": BOOLS, "has_links": BOOLS, "soil_on": BOOLS, "kernel": (AUTO, BASIC), "scheme": (GODUNOV, MUSCL, INERTIAL)},
                    lambda r: {"spec_wanted": int(old_spec_wanted(r))}),
    "tuner_on": ({"k.pair_tune": BOOLS, "math_mode": (FAST, STRICT), "k.two_step": (-1, 0, 1)}, lambda r: {"tuner_on": int(old_tuner_on(r))}),
    "sweep_alternates": ({"k.sweep_alternate": (-1, 0, 1), "precision": (8, 4), "scheme": (GODUNOV, MUSCL, INERTIAL)},
                         lambda r: {"sweep_alternates": int(old_sweep_alternates(r))}),
    "plan_single": ({"dynamic_dt": BOOLS, "scheme": (GODUNOV, MUSCL, INERTIAL), "kernel": (AUTO, BASIC), "quirks": (QUIRKS, QUIRKS & ~Q1), "f.use_alt": BOOLS,
                     "has_bdy": BOOLS, "bdy_on_ring": BOOLS, "f.edge_dirty": BOOLS, "f.need_full_reduce": BOOLS, "k.launch_tail": BOOLS,
                     "k.strip_reduce_always": BOOLS, "has_comm": BOOLS, "comm_world": (1, 2), "peer_direct": BOOLS, "strip_any_bdy": BOOLS, "strip_first": BOOLS,
                     "strip_any_full": BOOLS, "tail_allowed": BOOLS, "halo_overlap": BOOLS, "split_now": BOOLS, "has_tail_words": BOOLS}, old_step_begin),
    "tail_kind_for": ({"a.tail_want": BOOLS, "a.part_all": BOOLS, "a.own_stream": BOOLS, "a.blocks": (767, 768, 769, TAIL_MAX_BLOCKS, TAIL_MAX_BLOCKS + 1),
                       "k.tail_max_blocks": (768, TAIL_MAX_BLOCKS, 100000), "k.tail_max_blocks_k2k6": (500, 768, TAIL_MAX_BLOCKS), "a.push_now": BOOLS},
                      lambda r: {"tail_limit": old_tail_limit(r), "tail_limit_k2k6": old_tail_limit_k2k6(r),
                                 "tail_kind": old_make_tail_kind(r, old_tail_limit(r)), "tail_kind_k2k6": old_make_tail_kind(r, old_tail_limit_k2k6(r))}),
}
SAMPLE = 100000


def requests_of(inputs, seed):
    names = list(inputs)
    total = 1
    for n in names:
        total *= len(inputs[n])
    if total <= SAMPLE:
        return [dict(zip(names, combo)) for combo in itertools.product(*(inputs[n] for n in names))]
    rng = random.Random(seed)
    return [{n: rng.choice(inputs[n]) for n in names} for _ in range(SAMPLE)]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "plan_probe.cpp")])

    def run(requests, exe=str(exe)):
        """Every rule's answer to each request."""
        text = "".join(" ".join(f"{k}={int(v)}" for k, v in req.items()) + "\n" for req in requests)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
        out = r.stdout.splitlines()
        assert len(out) == len(requests)
        return [{k: int(v) for k, v in (w.split("=") for w in line.split())} for line in out]
    return run


def test_the_header_needs_no_hip_and_reads_no_environment():
    text = open(os.path.join(CSRC, "hp_plan.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in text.splitlines())
    assert "getenv" not in code and "#include <hip" not in code and "hip/" not in code
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", CSRC, os.path.join(HERE, "plan_probe.cpp")])


def test_the_moved_switches_are_named_in_plan_knobs_alone():
    """hp_engine.hip reads the once-per-process switches in plan_knobs() and nowhere else; hp_actors.hpp reads no environment at all."""
    engine = open(os.path.join(CSRC, "hp_engine.hip")).read()
    body = re.search(r"^const PlanKnobs& plan_knobs\(\)\n\{\n(.*?)^\}\n", engine, re.M | re.S).group(0)
    moved = ("HP_TWO_STEP", "HP_LAUNCH_TAIL", "HP_STRIP_REDUCE_ALWAYS", "HP_PAIR_BDY", "HP_PAIR_STRICT", "HP_PAIR_EXACT", "HP_PAIR_SKIP",
             "HP_FILL_AFTER_PAIRS", "HP_STRICT_SPECULATE", "HP_PAIR_TUNE", "HP_SWEEP_ALTERNATE", "HP_TAIL_MAX_BLOCKS", "HP_TAIL_MAX_BLOCKS_K2K6",
             "HP_MARCH2_RSEG", "HP_FUSE_BDY")
    rest = engine.replace(body, "")
    for name in moved:
        assert f'"{name}"' in body, name
        if name != "HP_MARCH2_RSEG":                         # (its VALUE is a tiling knob, read per domain by tiling_knobs)
            assert not re.search(r'getenv\("%s"\)' % name, rest) and not re.search(r'(num|has|on|off)\("%s"' % name, rest), name
    assert len(re.findall(r'"HP_MARCH2_RSEG"', rest)) == 1
    assert "getenv" not in "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, "hp_actors.hpp")).read().splitlines())


# ---- (a) rows written by hand from the parent's statements -----------------------------------------------------------------------------
PAIRS = {"k.two_step": 1}                                                    # an eligible fp64 FAST Godunov domain
READY = dict(PAIRS, **{"f.need_full_reduce": 0, "f.edge_dirty": 0})
RAIN = dict(PAIRS, has_bdy=1, fusable=1)
STRIP = dict(PAIRS, has_comm=1, comm_world=2, peer_direct=1, ghost_rows=2)
TAIL = {"tail_allowed": 1, "f.need_full_reduce": 0}                          # a single domain inside a batch call, its maximum remembered
STRIP_TAIL = dict(TAIL, has_comm=1, comm_world=2, peer_direct=1)
SPEC = {"k.strict_speculate": 1, "math_mode": STRICT}
HAND = [
    # each term of pairs_possible_common, flipped alone
    (PAIRS, {"pairs_possible_common": 1, "pairs_possible": 1}),
    ({}, {"pairs_possible_common": 0}), ({"march2_pays": 1}, {"pairs_possible_common": 1}), ({"k.two_step": 0, "march2_pays": 1}, {"pairs_possible_common": 0}),
    (dict(PAIRS, scheme=MUSCL), {"pairs_possible_common": 0}), (dict(PAIRS, scheme=INERTIAL), {"pairs_possible_common": 0}),
    (dict(PAIRS, kernel=BASIC), {"pairs_possible_common": 0}),
    (dict(PAIRS, has_bdy=1), {"pairs_possible_common": 0}), (RAIN, {"pairs_possible_common": 1}),
    (dict(RAIN, **{"k.pair_bdy": 0}), {"pairs_possible_common": 0}), (dict(RAIN, has_comm=1), {"pairs_possible_common": 0}),
    (dict(RAIN, comm_world=2), {"pairs_possible_common": 0}), (dict(RAIN, dynamic_dt=0), {"pairs_possible_common": 0}),
    (dict(PAIRS, quirks=QUIRKS & ~Q1), {"pairs_possible_common": 0}), (dict(PAIRS, quirks=QUIRKS & ~Q1, dynamic_dt=0), {"pairs_possible_common": 1}),
    (dict(PAIRS, **{"k.launch_tail": 0}), {"pairs_possible_common": 0}), (dict(PAIRS, has_tail_words=0), {"pairs_possible_common": 0}),
    (dict(PAIRS, rows=4), {"pairs_possible_common": 0}), (dict(PAIRS, cols=4), {"pairs_possible_common": 0}),
    # the fp32 boundary size threshold, and HP_TWO_STEP=1 overriding it
    ({"march2_pays": 1, "precision": 4, "has_bdy": 1, "fusable": 1, "cells": 29999999}, {"pairs_possible_common": 0}),
    ({"march2_pays": 1, "precision": 4, "has_bdy": 1, "fusable": 1, "cells": 30000000}, {"pairs_possible_common": 1}),
    ({"k.two_step": 1, "precision": 4, "has_bdy": 1, "fusable": 1, "cells": 29999999}, {"pairs_possible_common": 1}),
    ({"march2_pays": 1, "precision": 8, "has_bdy": 1, "fusable": 1, "cells": 29999999}, {"pairs_possible_common": 1}),
    # the STRICT leg: no boundaries, no communicator, dynamic timestep, not inside a speculative batch
    (dict(PAIRS, math_mode=STRICT), {"pairs_possible_common": 1}), (dict(PAIRS, math_mode=STRICT, **{"k.pair_strict": 0}), {"pairs_possible_common": 0}),
    (dict(RAIN, math_mode=STRICT), {"pairs_possible_common": 0}), (dict(PAIRS, math_mode=STRICT, has_comm=1), {"pairs_possible_common": 0}),
    (dict(PAIRS, math_mode=STRICT, comm_world=2), {"pairs_possible_common": 0}), (dict(PAIRS, math_mode=STRICT, dynamic_dt=0), {"pairs_possible_common": 0}),
    (dict(PAIRS, math_mode=STRICT, spec_now=1), {"pairs_possible_common": 0}), (dict(PAIRS, dynamic_dt=0), {"pairs_possible_common": 1}),
    # a single domain against a strip
    (dict(PAIRS, has_comm=1), {"pairs_possible_common": 1, "pairs_possible": 0}), (dict(PAIRS, comm_world=2), {"pairs_possible": 0}),
    (dict(PAIRS, peer_mine=1), {"pairs_possible": 0}), (dict(PAIRS, row_offset=2, global_rows=66), {"pairs_possible_common": 1, "pairs_possible": 0}),
    (dict(PAIRS, global_rows=128), {"pairs_possible_common": 1, "pairs_possible": 0}),
    # ... and the facts
    (PAIRS, {"pair_eligible": 0}), (READY, {"pair_eligible": 1}), (dict(READY, **{"f.use_alt": 1}), {"pair_eligible": 0}),
    (dict(READY, **{"f.rings_differ": 1}), {"pair_eligible": 0}), (dict(PAIRS, dynamic_dt=0), {"pair_eligible": 1}),
    (dict(READY, **{"k.two_step": 0}), {"pair_eligible": 0}),
    # what a strip can do
    (STRIP, {"strip_pairs_possible_here": 1, "pairs_possible": 0}), (dict(STRIP, ghost_rows=1), {"strip_pairs_possible_here": 0}),
    (dict(STRIP, ghost_rows=4), {"strip_pairs_possible_here": 0}), (dict(STRIP, peer_direct=0), {"strip_pairs_possible_here": 0}),
    (dict(STRIP, **{"f.rings_differ": 1}), {"strip_pairs_possible_here": 0}), (dict(STRIP, has_comm=0), {"strip_pairs_possible_here": 0}),
    (dict(STRIP, comm_world=1), {"strip_pairs_possible_here": 0}), (dict(STRIP, has_bdy=1, fusable=1), {"strip_pairs_possible_here": 0}),
    # the three-way cfl_mode table
    ({"scheme": MUSCL}, {"cfl_mode": 1, "edge_buffer": 1}), ({"quirks": QUIRKS & ~Q1}, {"cfl_mode": 1, "edge_buffer": 1, "reduce_buffer_is_primary": 0}),
    ({"f.use_alt": 1}, {"cfl_mode": 1, "edge_buffer": 0}), ({"has_bdy": 1}, {"cfl_mode": 2, "edge_buffer": 0, "boundaries_applied": 1}),
    ({}, {"cfl_mode": 0, "edge_buffer": 0, "reduce_buffer_is_primary": 1}), ({"scheme": MUSCL, "has_bdy": 1}, {"cfl_mode": 1, "boundaries_applied": 0}),
    ({"scheme": INERTIAL, "has_bdy": 1}, {"cfl_mode": 2}), ({"kernel": BASIC, "f.use_alt": 1}, {"cfl_mode": 0, "reduce_after": 1}),
    ({"kernel": BASIC, "scheme": INERTIAL, "f.use_alt": 1}, {"cfl_mode": 1}),            # (the basic kernel is the Godunov scheme's)
    ({"dynamic_dt": 0, "f.use_alt": 1}, {"cfl_mode": 0, "reduce_after": 0}), ({"dynamic_dt": 0, "has_bdy": 1}, {"cfl_mode": 0}),
    # reprice_ring: only with cfl_mode != 0, and with edge_dirty or a boundary on the ring
    ({}, {"reprice_ring": 0}), ({"f.use_alt": 1}, {"reprice_ring": 1}), ({"f.use_alt": 1, "f.edge_dirty": 0}, {"reprice_ring": 0}),
    ({"f.edge_dirty": 0, "has_bdy": 1, "bdy_on_ring": 1}, {"cfl_mode": 2, "reprice_ring": 1}), ({"f.edge_dirty": 0, "has_bdy": 1}, {"reprice_ring": 0}),
    ({"f.edge_dirty": 0, "bdy_on_ring": 1, "f.use_alt": 1}, {"reprice_ring": 0}), ({"has_bdy": 1, "bdy_on_ring": 1, "dynamic_dt": 0}, {"reprice_ring": 0}),
    ({"scheme": MUSCL, "has_bdy": 1, "bdy_on_ring": 1, "f.edge_dirty": 0}, {"reprice_ring": 0}),
    # the stand-alone reduction behind the launch
    ({}, {"reduce_after": 1}), ({"f.need_full_reduce": 0}, {"reduce_after": 0}), ({"f.use_alt": 1}, {"reduce_after": 0}),
    # tail_want, each of its eight terms flipped
    (TAIL, {"tail_want": 1}), (dict(TAIL, **{"k.launch_tail": 0}), {"tail_want": 0}), (dict(TAIL, tail_allowed=0), {"tail_want": 0}),
    (dict(TAIL, kernel=BASIC), {"tail_want": 0}), (dict(TAIL, **{"f.need_full_reduce": 1}), {"tail_want": 0}),
    (dict(TAIL, has_comm=1), {"tail_want": 1}), (dict(TAIL, has_comm=1, **{"k.strip_reduce_always": 1}), {"tail_want": 0}),
    (dict(TAIL, has_comm=1, comm_world=2), {"tail_want": 0}), (dict(TAIL, halo_overlap=1), {"tail_want": 0}),
    (dict(TAIL, halo_overlap=1, split_now=0), {"tail_want": 1}), (dict(TAIL, has_tail_words=0), {"tail_want": 0}),
    # tail_fresh 0 / 1 / 4 / 7
    (dict(TAIL, dynamic_dt=0), {"tail_fresh": 0, "tail_want": 1}), (TAIL, {"tail_fresh": 0}), (dict(TAIL, **{"f.use_alt": 1}), {"tail_fresh": 1, "tail_want": 1}),
    (STRIP_TAIL, {"tail_fresh": 4, "tail_want": 1}), (dict(STRIP_TAIL, **{"f.use_alt": 1}), {"tail_fresh": 7, "tail_want": 1}),
    (dict(STRIP_TAIL, strip_any_bdy=1), {"tail_fresh": 7, "tail_want": 0}), (dict(STRIP_TAIL, strip_any_full=1), {"tail_fresh": 4, "tail_want": 1}),
    (dict(STRIP_TAIL, strip_any_full=1, strip_first=1), {"tail_fresh": 7, "tail_want": 0}), (dict(STRIP_TAIL, dynamic_dt=0), {"tail_fresh": 4, "tail_want": 1}),
    # do all strips reduce
    ({}, {"strips_reduce_everyone": 0}), ({"f.use_alt": 1}, {"strips_reduce_everyone": 1}), ({"strip_any_bdy": 1}, {"strips_reduce_everyone": 1}),
    ({"strip_any_full": 1}, {"strips_reduce_everyone": 0}), ({"strip_any_full": 1, "a.first_of_batch": 1}, {"strips_reduce_everyone": 1}),
    ({"a.first_of_batch": 1}, {"strips_reduce_everyone": 0}), ({"scheme": MUSCL}, {"strips_reduce_everyone": 1}), ({"kernel": BASIC}, {"strips_reduce_everyone": 1}),
    ({"quirks": QUIRKS & ~Q1}, {"strips_reduce_everyone": 1}), ({"f.use_alt": 1, "dynamic_dt": 0}, {"strips_reduce_everyone": 0}),
    # fill_wanted: off with stamps present
    ({"f.other_stale": 1}, {"fill_wanted": 1}), ({}, {"fill_wanted": 0}), ({"f.other_stale": 1, "k.fill_after_pairs": 0}, {"fill_wanted": 0}),
    ({"f.other_stale": 1, "has_stamps": 1, "bdy_removes_water": 1}, {"fill_wanted": 0}), ({"f.other_stale": 1, "has_stamps": 1}, {"fill_wanted": 1}),
    ({"f.other_stale": 1, "has_stamps": 1, "math_mode": STRICT}, {"fill_wanted": 0}), ({"f.other_stale": 1, "bdy_removes_water": 1}, {"fill_wanted": 1}),
    ({"f.other_stale": 1, "scheme": MUSCL}, {"fill_wanted": 0}), ({"f.other_stale": 1, "kernel": BASIC}, {"fill_wanted": 0}),
    # pair_records
    ({}, {"pair_records": 1}), ({"precision": 4}, {"pair_records": 0}), ({"a.strip": 1}, {"pair_records": 0}), ({"has_bdy": 1}, {"pair_records": 0}),
    ({"a.exact": 1}, {"pair_records": 0}), ({"math_mode": STRICT}, {"pair_records": 0}), ({"a.tile_rows": 33}, {"pair_records": 0}),
    ({"a.tile_rows": 32}, {"pair_records": 1}), ({"k.pair_skip": 0}, {"pair_records": 0}),
    # spec_wanted
    (SPEC, {"spec_wanted": 1}), (dict(SPEC, has_links=1), {"spec_wanted": 0}), (dict(SPEC, soil_on=1), {"spec_wanted": 0}), (dict(SPEC, has_comm=1), {"spec_wanted": 0}),
    (dict(SPEC, fusable=1), {"spec_wanted": 0}), (dict(SPEC, fusable=1, spec_fused_kept=1), {"spec_wanted": 1}), (dict(SPEC, **{"a.n": 7}), {"spec_wanted": 0}),
    (dict(SPEC, precision=4), {"spec_wanted": 0}), (dict(SPEC, scheme=INERTIAL), {"spec_wanted": 0}), (dict(SPEC, scheme=MUSCL), {"spec_wanted": 1}),
    (dict(SPEC, kernel=BASIC), {"spec_wanted": 0}), ({"math_mode": STRICT}, {"spec_wanted": 0}), ({"k.strict_speculate": 1}, {"spec_wanted": 0}),
    # pair_exact: forced both ways, always for STRICT, by default only with a boundary that removes water
    ({}, {"pair_exact": 0}), ({"bdy_removes_water": 1}, {"pair_exact": 1}), ({"k.pair_exact": 1}, {"pair_exact": 1}),
    ({"k.pair_exact": 0, "bdy_removes_water": 1}, {"pair_exact": 0}), ({"k.pair_exact": 0, "math_mode": STRICT}, {"pair_exact": 1}), ({"math_mode": STRICT}, {"pair_exact": 1}),
    # the STRICT 12-row cap, the tuner, the sweep direction, the tail block's limit
    ({"math_mode": STRICT}, {"pair_tile_rows": 12}), ({"math_mode": STRICT, "k.march2_rseg_forced": 1}, {"pair_tile_rows": 24}), ({}, {"pair_tile_rows": 24}),
    ({"math_mode": STRICT, "a.march2_rseg": 8}, {"pair_tile_rows": 8}),
    ({"math_mode": STRICT}, {"tuner_on": 1}), ({}, {"tuner_on": 0}), ({"math_mode": STRICT, "k.two_step": 1}, {"tuner_on": 0}),
    ({"math_mode": STRICT, "k.two_step": 0}, {"tuner_on": 1}), ({"math_mode": STRICT, "k.pair_tune": 0}, {"tuner_on": 0}),
    ({}, {"sweep_alternates": 0}), ({"precision": 4}, {"sweep_alternates": 1}), ({"scheme": MUSCL}, {"sweep_alternates": 1}), ({"scheme": INERTIAL}, {"sweep_alternates": 0}),
    ({"k.sweep_alternate": 1}, {"sweep_alternates": 1}), ({"k.sweep_alternate": 0, "precision": 4}, {"sweep_alternates": 0}),
    ({}, {"tail_kind": 1, "tail_kind_k2k6": 1, "tail_limit": TAIL_MAX_BLOCKS}), ({"a.push_now": 1}, {"tail_kind": 2}), ({"a.tail_want": 0}, {"tail_kind": 0}),
    ({"a.part_all": 0}, {"tail_kind": 0}), ({"a.own_stream": 0, "a.push_now": 1}, {"tail_kind": 0}), ({"a.blocks": TAIL_MAX_BLOCKS}, {"tail_kind": 1}),
    ({"a.blocks": TAIL_MAX_BLOCKS + 1}, {"tail_kind": 0}), ({"a.blocks": TAIL_MAX_BLOCKS + 1, "k.tail_max_blocks": 100000}, {"tail_kind": 0, "tail_limit": TAIL_MAX_BLOCKS}),
    ({"a.blocks": 769, "k.tail_max_blocks": 768}, {"tail_kind": 0, "tail_kind_k2k6": 0}), ({"a.blocks": 768, "k.tail_max_blocks": 768}, {"tail_kind": 1, "tail_kind_k2k6": 1}),
    ({"a.blocks": 769, "k.tail_max_blocks_k2k6": 768}, {"tail_kind": 1, "tail_kind_k2k6": 0, "tail_limit_k2k6": 768}),
]


def test_rows_written_by_hand(probe):
    for (req, want), got in zip(HAND, probe([req for req, _ in HAND])):
        assert {k: got[k] for k in want} == want, req


def test_the_transcriptions_agree_with_the_rows_written_by_hand():
    """(so that a slip of the pen in either shows without the probe)"""
    for req, want in HAND:
        r = complete(req)
        got = {}
        for _, old in RULES.values():
            got.update(old(r))
        got["strips_reduce_everyone"] = int(old_everyone_allreduce(r) or False)
        assert {k: got[k] for k in want} == want, req


@pytest.mark.parametrize("rule", list(RULES))
def test_rule_against_the_parents_expression(probe, rule):
    inputs, old = RULES[rule]
    requests = requests_of(inputs, seed=rule) + [req for req, _ in HAND]
    for req, got in zip(requests, probe(requests)):
        want = old(complete(req))
        assert {k: got[k] for k in want} == want, req


def test_the_two_old_copies_of_do_all_strips_reduce_never_differed(probe):
    """step_begin_impl's copy (with d->strip_first) decided whether the tail block may stand in for the reduction, strip_allreduce_max's
    (with first_of_batch) whether the rank enters it: hp_strip_step_batch sets strip_first = (i == 0) and passes i == 0.  The second copy
    sat behind `if (!dynamic_dt) return`: rows with a fixed timestep never reached it."""
    inputs = {"dynamic_dt": BOOLS, "scheme": (GODUNOV, MUSCL, INERTIAL), "kernel": (AUTO, BASIC), "quirks": (QUIRKS, QUIRKS & ~Q1), "f.use_alt": BOOLS,
              "strip_any_bdy": BOOLS, "strip_any_full": BOOLS, "first": BOOLS}
    requests = [dict({k: v for k, v in req.items() if k != "first"}, **{"strip_first": req["first"], "a.first_of_batch": req["first"]})
                for req in requests_of(inputs, seed=0)]
    assert len(requests) == 2 * 3 * 2 * 2 * 2 * 2 * 2 * 2
    for req, got in zip(requests, probe(requests)):
        r = complete(req)
        a, b = old_everyone_step_begin(r), old_everyone_allreduce(r)
        assert b is None or a == b, req
        assert got["strips_reduce_everyone"] == int(a), req


def test_the_probe_runs_clean_under_the_sanitizers(probe, tmp_path):
    exe = tmp_path / "plan_probe_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-I", CSRC, "-o", str(exe),
                           os.path.join(HERE, "plan_probe.cpp")])
    requests = [req for req, _ in HAND] + requests_of(RULES["plan_single"][0], seed="san")[:2000]
    assert probe(requests, exe=str(exe)) == probe(requests)
