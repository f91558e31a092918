"""The host protocol around SGPRModel.md_run — batch size, gate, `final`, which rows log and count, the hand-over, the frame
record's cap — as run_md, run_relax and run_neb speak it to a scripted engine (loop_trace.py), against the traces recorded
before the three methods shared autoforce_amd/device_loop.py (tests/golden/g18_loop_trace.json): the calls on the engine with
their scalar arguments and rows of deviates, every yield and callback with calc.step and the atoms, the log, the returned
dicts and the exceptions, compared for equality.
Not covered here: a bias (md_meta*: a stand-in Meta is no cheaper than the real one; tests/test_hip_meta_callers.py and
test_meta_twin_cpu.py hold it) and the host-loop fallbacks, which the twins' own tests drive."""
import json
import os

import pytest

from conftest import GOLDEN
from loop_trace import scenarios

with open(os.path.join(GOLDEN, "g18_loop_trace.json")) as _f:
    EXPECTED = json.load(_f)
SCENARIOS = scenarios()


def test_every_recorded_scenario_is_still_run():
    assert sorted(SCENARIOS) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_trace_is_what_it_was(name):
    got = json.loads(json.dumps(SCENARIOS[name]()))
    want = EXPECTED[name]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: entry {k} of the trace"
    assert len(got) == len(want)


def test_the_scenarios_reach_what_they_are_for():
    """The script places halts where the names say: read back from the recorded traces."""
    def calls(name, what):
        return [e for e in EXPECTED[name] if e[0] == what]
    # a halt on the first row of a batch hands over with no row accepted before it; on the last, with the whole batch
    assert [e[1] for e in calls("md_langevin_rng_first_row", "calculate")] == [8]
    assert [e[1] for e in calls("md_langevin_rng_consecutive", "calculate")] == [3, 4]
    assert [e[1] for e in calls("md_langevin_rng_final", "calculate")] == [30]
    assert not calls("md_langevin_rng_never", "calculate")
    assert sorted(n for n in EXPECTED if calls(n, "raise")) == ["md_barostat_needs_thermostat", "md_barostat_refuses_constraints", "neb_no_interior_image"]
    # the batch grows 8, 16, 32; a halt sets it back to 8, which the single re-evaluation — a call that ran through — doubles
    assert [e[1] for e in calls("md_langevin_rng_growing_batch", "md_run")] == [8, 1, 16, 1, 16, 32, 1, 16, 24, 1]
    # deviates: a `final` call draws one row fewer and is zero-padded
    last = calls("md_langevin_rng_never", "md_run")[-1]
    assert last[4] is True and last[2][-1] == 0.0 and last[2][-2] == 30.0
    # the frame record's cap
    assert max(e[1] for e in calls("md_sync3_record_max1", "md_run")) == 3 and max(e[1] for e in calls("md_sync3_record_max2", "md_run")) == 6
    assert not calls("md_attached", "md_record") and calls("md_attached", "_md_attached_done") == [["_md_attached_done", ["a", "b"]]]
    assert len(calls("md_filter", "md_filter_push")) == 4 and calls("md_filter", "filter")[0][3] == 4
    assert calls("md_empty_model", "calculate")[0][1] == 0 and calls("md_empty_model", "md_run")[0][1:4] == [1, [[1, 2, 3], 1.0], 0.0]
    assert len(calls("relax_clearTrue_grow1", "relax_reset")) == 5 and not calls("relax_clearTrue_grow0", "relax_reset")
    assert not calls("relax_clearFalse_grow1", "relax_reset")
    assert [e[1] for e in calls("relax_frames_max1", "on_frame")] == [0, 3, 6, 9, 12, 15, 18, 21, 24, 27, 30, 31]
    assert len(calls("neb_halts_grow1", "neb_reset")) == 5 and not calls("neb_halts_grow0", "neb_reset")
    assert {e[1] for e in calls("neb_halts_grow1", "neb_state") if e[2]} == {0, -1}
