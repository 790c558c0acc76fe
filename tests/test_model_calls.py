"""Model's side of the engine's surface, pinned: on one 40 x 32 model file with every feature on (tests/model_calls.py), the calls the
engine receives -- names, order, arguments --, the log lines and the bytes of every output file equal what the front end produced
before Model.__init__ and write_outputs were split into one method per feature (tests/model_calls_expected.json, written by
`python tests/model_calls.py cpu` at that commit).  Three runs: the host paths, the device paths, and a single tracer in the set's place."""
import json
import os

import pytest

import model_calls as MC

with open(os.path.join(MC.HERE, "model_calls_expected.json")) as f:
    EXPECTED = json.load(f)


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    return MC.cpu_records(tmp_path_factory.mktemp("model_calls"))


def test_the_model_file_turns_everything_on(records):
    assert set(records) == set(EXPECTED) == set(MC.CPU_CASES)
    for name, r in records.items():
        called = {c[0] for c in r["calls"]}
        assert "error" not in r and {"add_uniform", "add_links", "add_open", "add_infiltration", "tracer_add_source", "infiltration_read", "tracer_read",
                                     "links_read", "open_read", "stats"} <= called, name
        assert ("tracer_enable" in called) == (name == "single") and ({"tracer_enable_set", "tracer_set_exchange", "tracer_deposit_read"} <= called) == (name != "single")
        device = {"derive", "peaks_enable", "peaks_sample", "peaks", "probes_enable", "probes_sample", "probes", "zones_enable", "zones_sample", "zones",
                  "overview", "sparse", "bed_shape_add", "bed_apply"}
        assert device <= called if name == "device" else not device & called, name
        assert len([n for n in r["files"] if n.startswith("depth_max4_")]) == 2 and len([n for n in r["files"] if n.endswith(".npz")]) == 2
        assert {"gauges.csv", "sections.csv", "zones.csv", "links.csv", "outflow.csv"} <= set(r["files"])


@pytest.mark.parametrize("name", sorted(MC.CPU_CASES))
def test_the_engine_sees_the_same_calls(records, name):
    got, want = records[name]["calls"], EXPECTED[name]["calls"]
    assert [c[0] for c in got] == [c[0] for c in want]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g[0])


@pytest.mark.parametrize("name", sorted(MC.CPU_CASES))
def test_the_same_files_with_the_same_bytes(records, name):
    assert sorted(records[name]["files"]) == sorted(EXPECTED[name]["files"])
    for n, d in records[name]["files"].items():
        assert d == EXPECTED[name]["files"][n], n
    assert records[name]["log"] == EXPECTED[name]["log"]
