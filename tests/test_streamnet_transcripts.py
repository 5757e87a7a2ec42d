"""bin/streamnet's error runs (a src file that is missing, a p raster of another size, the -net layer that is not written) reproduce
tests/golden/tool_transcripts_streamnet.json: exit status, stdout and stderr, and no output file.  They end before the compute step and need no GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tool_transcripts_streamnet.json")


def load_script():
    spec = importlib.util.spec_from_file_location("streamnet_transcripts", os.path.join(ROOT, "scripts", "streamnet_transcripts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_error_runs_reproduce_the_recorded_transcripts():
    st = load_script()
    expected = st.load_fixture(FIXTURE, "err")
    assert len(expected) == 3 and all(not any(e["files"].values()) for e in expected.values())
    e = expected["err/streamnet/missing_src"]       # the ToolRun frame's status for a file it cannot read (TDX_ERR_FILE)
    assert e["status"] == 21 and "Error opening file" in e["stdout"]
    e = expected["err/streamnet/p_of_another_size"]   # the reference's words and its MPI_Abort code (src/streamnet.cpp:427-431)
    assert e["status"] == 4 and e["stdout"].endswith("pfile and src files not the same size. Exiting \n") and "This run may take on the order of" in e["stderr"]
    e = expected["err/streamnet/net_refused"]       # refused before the banner
    assert e["status"] == 2 and e["stdout"] == "" and "-net" in e["stderr"]
    bad = st.differences(expected, st.collect("err"))
    assert not bad, "\n".join(bad)
