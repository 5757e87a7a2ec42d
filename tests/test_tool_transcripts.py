"""The tools' error paths that end before a GPU context exists (a missing input, an input of another size at every comparison
site under each mismatch policy, the early exits) reproduce tests/golden/tool_transcripts.json: exit status, stdout, stderr
and which output files exist.  The fixture is scripts/tool_transcripts.py --record on a build of commit 1e7abfb, the last one
before the file-level tool functions moved onto one frame."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tool_transcripts.json")


def load_script():
    spec = importlib.util.spec_from_file_location("tool_transcripts", os.path.join(ROOT, "scripts", "tool_transcripts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_error_runs_reproduce_the_recorded_transcripts():
    tt = load_script()
    expected = tt.load_fixture(FIXTURE, "err")
    assert len(expected) >= 60                                   # 22 missing inputs, 30 comparison sites, the early exits
    assert {e["status"] for e in expected.values()} >= {0, 5, 21, 41}
    bad = tt.differences(expected, tt.collect("err"))
    assert not bad, "\n".join(bad)
