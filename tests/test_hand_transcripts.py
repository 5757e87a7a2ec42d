"""The two HAND tools' error runs (a missing catchment list, a list with two columns) reproduce tests/golden/tool_transcripts_hand.json: exit
status, stdout and stderr.  They end before the compute step and need no GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tool_transcripts_hand.json")


def load_script():
    spec = importlib.util.spec_from_file_location("hand_transcripts", os.path.join(ROOT, "scripts", "hand_transcripts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_error_runs_reproduce_the_recorded_transcripts():
    ht = load_script()
    expected = ht.load_fixture(FIXTURE, "err")
    assert len(expected) == 2
    assert "ERROR: Cannot open catch list file!" in expected["err/catchhydrogeo/no_list"]["stderr"]
    assert "at least 3 columns" in expected["err/catchhydrogeo/two_columns"]["stderr"]
    bad = ht.differences(expected, ht.collect("err"))
    assert not bad, "\n".join(bad)
