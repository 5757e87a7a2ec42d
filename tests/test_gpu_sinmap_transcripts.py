"""bin/sinmapsi with --gpus 1 and --gpus 2 in its three argument forms reproduces tests/golden/tool_transcripts_sinmap.json: exit status, stdout (the
banner, the two times; blanked), stderr (the reference's run-time estimate) and the SHA-256 of the two rasters.  The fixture is
scripts/sinmap_transcripts.py --record on the build that introduced the tool.  Cells are independent, so one and two strips write the same files, and
the 12-argument form and the flag form are the same run."""
import pytest

from test_sinmap_transcripts import FIXTURE, load_script

pytestmark = pytest.mark.gpu


def test_gpu_runs_reproduce_the_recorded_transcripts():
    st = load_script()
    expected = st.load_fixture(FIXTURE, "gpu")
    assert len(expected) == 6 and all(e["status"] == 0 and all(e["files"].values()) for e in expected.values())
    assert all("SinmapSI version" in e["stdout"] and "Compute time: T" in e["stdout"] and "File write time: T" in e["stdout"] for e in expected.values())
    for tag in ("pos10", "pos12", "flags"):
        assert expected[f"gpu1/plain/sinmapsi/{tag}"]["files"] == expected[f"gpu2/plain/sinmapsi/{tag}"]["files"]
    assert expected["gpu1/plain/sinmapsi/pos12"]["files"] == expected["gpu1/plain/sinmapsi/flags"]["files"] != expected["gpu1/plain/sinmapsi/pos10"]["files"]
    bad = st.differences(expected, st.collect("gpu"))
    assert not bad, "\n".join(bad)
