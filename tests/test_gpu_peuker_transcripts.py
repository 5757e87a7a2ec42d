"""bin/peukerdouglas with --gpus 1 and --gpus 2, the default weights and a -par, reproduces tests/golden/tool_transcripts_peuker.json: exit status, stdout
(the banner, the footer; times blanked), stderr (the reference's run-time estimate) and the SHA-256 of the stream-source raster.  The fixture is
scripts/peuker_transcripts.py --record on the build that introduced the tool.  The output is exact, so one and two strips write the same file."""
import pytest

from test_peuker_transcripts import FIXTURE, load_script

pytestmark = pytest.mark.gpu


def test_gpu_runs_reproduce_the_recorded_transcripts():
    pt = load_script()
    expected = pt.load_fixture(FIXTURE, "gpu")
    assert len(expected) == 4 and all(e["status"] == 0 and all(e["files"].values()) for e in expected.values())
    assert all("PeukerDouglas version" in e["stdout"] and "Processors: " in e["stdout"] for e in expected.values())
    for tag in ("default", "par"):
        assert expected[f"gpu1/plain/peukerdouglas/{tag}"]["files"] == expected[f"gpu2/plain/peukerdouglas/{tag}"]["files"]
    bad = pt.differences(expected, pt.collect("gpu"))
    assert not bad, "\n".join(bad)
