"""The engine calls and the use of the random streams of the five ``*_with_nowcasts`` functions
against a recorded trace.

tests/scenario_trace.py calls each of them from a fresh copy of one fitted snapshot, in every mode
(default, resampling forced and partial, the three refinement modes, scenarios on differing dates,
the invalid calls) on four host engines (no sampler; the sampler; sampler, independent sampler,
targets and scores; those plus a resident factor), and writes down the engine's and the factor's
method calls with the shapes of their arguments and the sampler's seeds, where every random stream
— the base model's and every scenario clone's — stands afterwards, and the exception type of a call
that raises.  The record must equal tests/golden/scenario_trace_v1.json: the code of nowcast.py may
be rearranged, what a call asks of the engine and takes from the streams, and in which order, may
not change.  The golden file holds names, shapes and integers only; it is regenerated
(``python -m tests.scenario_trace --record tests/golden/scenario_trace_v1.json``) only by a change
that means to move a call or a draw."""
import json
import os

from tests import scenario_trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenario_trace_v1.json")


def test_scenario_trace_equals_the_recorded_one():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(scenario_trace.record()))
    assert sorted(got) == sorted(want)
    for label in sorted(want):
        g, w = got[label], want[label]
        assert g["raised"] == w["raised"], label
        k = next((i for i, (a, b) in enumerate(zip(g["calls"], w["calls"])) if a != b),
                 min(len(g["calls"]), len(w["calls"])))
        assert g["calls"] == w["calls"], (
            f"{label}: call {k} of {len(g['calls'])} (recorded: {len(w['calls'])}): "
            f"got {g['calls'][k] if k < len(g['calls']) else '<end>'}, "
            f"want {w['calls'][k] if k < len(w['calls']) else '<end>'}")
        assert g["streams"] == w["streams"], f"{label}: a random stream stands elsewhere"
