"""The launch decisions did not move when they moved house (hp_plan.hpp): tests/plan_counts_worker.py's scenarios -- every kernel family,
pairs with and without boundaries, exact and STRICT pairs, the size threshold of fp32, the switches HP_LAUNCH_TAIL and
HP_FILL_AFTER_PAIRS, a grid loaded block-wise, split steps and a checkpoint between batches -- leave the launch counts, pair counts,
iteration counts and bits that tests/plan_counts_expected.json holds.  That file was recorded by the same worker on the commit named
inside it, the one BEFORE the decisions were gathered: the expectation never comes from the code under test.  Every field is compared
for equality; each scenario is a child process with its own time limit."""
import json
import os

import pytest

import plan_counts_worker as worker

pytestmark = pytest.mark.gpu
EXPECTED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_counts_expected.json")))


def test_the_recording_covers_the_workers_scenarios():
    assert set(EXPECTED["scenarios"]) == set(worker.SCENARIOS) and len(EXPECTED["commit"]) >= 7


@pytest.mark.parametrize("scenario", list(worker.SCENARIOS))
def test_launch_decisions_are_the_recorded_ones(scenario):
    got, want = worker.run_child(scenario, timeout=120), EXPECTED["scenarios"][scenario]
    assert got["trail"] == want["trail"]
    assert got["sha256"] == want["sha256"]
    assert got == want
