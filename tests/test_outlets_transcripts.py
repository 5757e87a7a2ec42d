"""The error runs of bin/moveoutletstostrm and bin/connectdown (a raster or an outlet source that is missing, a raster of another size, an output
extension no layer writer exists for) reproduce tests/golden/tool_transcripts_outlets.json: exit status, stdout and stderr, and no output file.
They end before the compute step and need no GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tool_transcripts_outlets.json")


def load_script():
    spec = importlib.util.spec_from_file_location("outlets_transcripts", os.path.join(ROOT, "scripts", "outlets_transcripts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_error_runs_reproduce_the_recorded_transcripts():
    ot = load_script()
    expected = ot.load_fixture(FIXTURE, "err")
    assert len(expected) == 8 and all(not any(e["files"].values()) for e in expected.values())
    e = expected["err/moveoutletstostrm/missing_src"]            # the ToolRun frame's status for a file it cannot read (TDX_ERR_FILE)
    assert e["status"] == 21 and e["stdout"].startswith("MoveOutletsToStreams version ") and "Error opening file" in e["stdout"]
    e = expected["err/moveoutletstostrm/p_of_another_size"]      # the reference's words and its MPI_Abort code (src/MoveOutletsToStrm.cpp:153-157)
    assert e["status"] == 4 and e["stdout"].endswith("src and p files not the same size. Exiting \n") and "This run may take on the order of" in e["stderr"]
    e = expected["err/moveoutletstostrm/missing_outlets"]        # :184-188, exit(1)
    assert e["status"] == 1 and "Error Opening datasource " in e["stdout"]
    e = expected["err/moveoutletstostrm/kml_refused"]            # refused before the banner, with the two kinds that are written
    assert e["status"] == 2 and e["stdout"] == "" and ".shp" in e["stderr"] and ".geojson" in e["stderr"]
    e = expected["err/connectdown/missing_w"]
    assert e["status"] == 21 and e["stdout"].startswith("ConnectDown version ")
    e = expected["err/connectdown/p_of_another_size"]            # src/ConnectDown.cpp:144-148
    assert e["status"] == 4 and e["stdout"].endswith("w and p files not the same size. Exiting \n")
    e = expected["err/connectdown/ad8_of_another_size"]          # :167-171
    assert e["status"] == 4 and e["stdout"].endswith("ad8 and w files not the same size. Exiting \n")
    e = expected["err/connectdown/sqlite_refused"]
    assert e["status"] == 2 and e["stdout"] == "" and "od.sqlite" in e["stderr"]
    bad = ot.differences(expected, ot.collect("err"))
    assert not bad, "\n".join(bad)
