"""bin/dropanalysis' error runs (one threshold, a missing outlet file, an outlet on a cell without a direction, a direction raster of another
size) reproduce tests/golden/tool_transcripts_dropan.json: exit status, stdout and stderr, and no table.  They end before the
compute step and need no GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tool_transcripts_dropan.json")


def load_script():
    spec = importlib.util.spec_from_file_location("dropan_transcripts", os.path.join(ROOT, "scripts", "dropan_transcripts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_error_runs_reproduce_the_recorded_transcripts():
    dt = load_script()
    expected = dt.load_fixture(FIXTURE, "err")
    assert len(expected) == 4 and all(e["files"] == {"drp.txt": None} for e in expected.values())
    assert "Number of thresholds must be greater than 1." in expected["err/dropanalysis/one_threshold"]["stdout"]
    assert expected["err/dropanalysis/missing_outlets"]["status"] == 5 and "Error opening shapefile. Exiting" in expected["err/dropanalysis/missing_outlets"]["stdout"]
    assert "lies on a cell without a flow direction" in expected["err/dropanalysis/outlet_without_direction"]["stderr"]
    assert "dir and ssa files not the same size. Exiting" in expected["err/dropanalysis/small_p"]["stdout"]
    bad = dt.differences(expected, dt.collect("err"))
    assert not bad, "\n".join(bad)
