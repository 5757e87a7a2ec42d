"""bin/streamnet without outlets, with outlets, with -sw and with -v, and with --gpus 2 and --gpus 5, reproduces tests/golden/tool_transcripts_streamnet.json: exit status, stdout (the
banner, the reads in the reference's order, the footer; times blanked), stderr (the reference's run-time estimate and its three progress lines) and the
SHA-256 of the four outputs.  The fixture is scripts/streamnet_transcripts.py --record on the build that introduced the tool; the outputs themselves are
held to the reference by tests/test_gpu_streamnet.py."""
import pytest

from test_streamnet_transcripts import FIXTURE, load_script

pytestmark = pytest.mark.gpu


def test_gpu_runs_reproduce_the_recorded_transcripts():
    st = load_script()
    expected = st.load_fixture(FIXTURE, "gpu")
    assert len(expected) == 6 and all(e["status"] == 0 and all(e["files"].values()) for e in expected.values())
    for e in expected.values():
        assert e["stdout"].startswith("StreamNet version ") and "\nRead time: T\nLength compute time: T\nLink compute time: T\n" in e["stdout"]
        assert "Evaluating distances to outlet\nCreating links\n\n Calculating watersheds\n" in e["stderr"]
    assert expected["gpu1/holes/streamnet/verbose"]["files"] == expected["gpu1/holes/streamnet/outlets"]["files"]
    assert "Process: 0, numOutlets: 7\n" in expected["gpu1/holes/streamnet/verbose"]["stdout"]
    assert expected["gpu1/holes/streamnet/plain"]["files"]["ord.tif"] == expected["gpu1/holes/streamnet/sw"]["files"]["ord.tif"]
    for gpus, tag in ((2, "outlets"), (5, "sw")):   # strips write the same four files
        assert expected[f"gpu{gpus}/holes/streamnet/{tag}"]["files"] == expected[f"gpu1/holes/streamnet/{tag}"]["files"]
        assert f"Processors: {gpus}\n" in expected[f"gpu{gpus}/holes/streamnet/{tag}"]["stdout"]
    assert "Processors: 1\n" in expected["gpu1/holes/streamnet/plain"]["stdout"]
    bad = st.differences(expected, st.collect("gpu"))
    assert not bad, "\n".join(bad)
