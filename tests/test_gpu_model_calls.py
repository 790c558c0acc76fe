"""tests/test_model_calls.py on the HIP engine: the recording proxy around a real Domain, a fixed batch size, the call log and the list
of output files against tests/model_calls_expected_gpu.json (`python tests/model_calls.py gpu` at the commit in front of the front
end's split).  The engine carries a tracer OR links and an infiltration, so the file with everything on is followed up to that
refusal and then once per side, and once more with a single tracer."""
import json
import os

import pytest

import model_calls as MC

pytestmark = pytest.mark.gpu

with open(os.path.join(MC.HERE, "model_calls_expected_gpu.json")) as f:
    EXPECTED = json.load(f)


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    return MC.gpu_records(tmp_path_factory.mktemp("model_calls_gpu"))


def test_the_cases_cover_every_feature(records):
    assert set(records) == set(EXPECTED) == set(MC.GPU_CASES)
    assert "hp_tracer_enable_set" in records["everything"]["error"] and [n for n in records if "error" in records[n]] == ["everything"]
    called = {name: {c[0] for c in r["calls"]} for name, r in records.items()}
    assert {"add_links", "add_open", "add_infiltration", "tracer_enable_set"} <= called["everything"]
    assert {"add_uniform", "add_links", "add_open", "add_infiltration", "infiltration_read", "links_read", "open_read"} <= called["water"]
    assert {"tracer_enable_set", "tracer_add_source", "tracer_set_exchange", "tracer_read", "tracer_deposit_read"} <= called["tracers"]
    assert "tracer_enable" in called["single"]
    for name in ("water", "tracers", "single"):
        assert {"derive", "peaks_enable", "peaks_sample", "peaks", "probes_enable", "probes_sample", "probes", "zones_enable", "zones_sample", "zones",
                "overview", "sparse", "bed_shape_add", "bed_apply", "stats"} <= called[name], name


@pytest.mark.parametrize("name", sorted(MC.GPU_CASES))
def test_the_engine_sees_the_same_calls(records, name):
    got, want = records[name]["calls"], EXPECTED[name]["calls"]
    assert [c[0] for c in got] == [c[0] for c in want]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g[0])
    assert records[name].get("error") == EXPECTED[name].get("error")
    assert sorted(records[name]["files"]) == sorted(EXPECTED[name]["files"])
