"""bin/peukerdouglas' error runs (an input file that is missing, one that is no TIFF) reproduce tests/golden/tool_transcripts_peuker.json: exit status,
stdout and stderr, and no output raster.  They end before the compute step and need no GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tool_transcripts_peuker.json")


def load_script():
    spec = importlib.util.spec_from_file_location("peuker_transcripts", os.path.join(ROOT, "scripts", "peuker_transcripts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_error_runs_reproduce_the_recorded_transcripts():
    pt = load_script()
    expected = pt.load_fixture(FIXTURE, "err")
    assert len(expected) == 2 and all(e["files"] == {"ss.tif": None} for e in expected.values())
    for e in expected.values():   # the ToolRun frame's status for a file it cannot read (TDX_ERR_FILE, the reference's MPI_Abort code) is the exit status
        assert e["status"] == 21 and "Error opening file" in e["stdout"]
    bad = pt.differences(expected, pt.collect("err"))
    assert not bad, "\n".join(bad)
