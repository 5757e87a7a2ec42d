"""bin/sinmapsi's error runs (an unreadable -calpar, a slope file that is missing, a contributing-area raster of another size) reproduce
tests/golden/tool_transcripts_sinmap.json: exit status, stdout and stderr, and no output raster.  They end before the compute step and need no GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tool_transcripts_sinmap.json")


def load_script():
    spec = importlib.util.spec_from_file_location("sinmap_transcripts", os.path.join(ROOT, "scripts", "sinmap_transcripts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_error_runs_reproduce_the_recorded_transcripts():
    st = load_script()
    expected = st.load_fixture(FIXTURE, "err")
    assert len(expected) == 3 and all(e["files"] == {"si.tif": None, "sat.tif": None} for e in expected.values())
    # the reference's main prints the code and returns 0 for 15 (unreadable -calpar) and 1 (dimensions); a file the frame cannot read is its status 21
    assert expected["err/sinmapsi/missing_calpar"]["status"] == 0 and "Sinmap Stability Index Error 15" in expected["err/sinmapsi/missing_calpar"]["stdout"]
    assert expected["err/sinmapsi/small_sca"]["status"] == 0 and "files have different dimensions" in expected["err/sinmapsi/small_sca"]["stderr"]
    assert expected["err/sinmapsi/missing_slp"]["status"] == 21
    bad = st.differences(expected, st.collect("err"))
    assert not bad, "\n".join(bad)
