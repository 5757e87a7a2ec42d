"""bin/dropanalysis with --gpus 1 and --gpus 2 and both step types reproduces tests/golden/tool_transcripts_dropan.json: exit status, stdout (the banner,
the console table, the optimum line; times blanked), stderr (the reference's run-time estimate) and the SHA-256 of the table.  The fixture is
scripts/dropan_transcripts.py --record on the build that introduced the tool.  The fp64 sums are added in a fixed order, so each run's table is
reproducible; two strips add in another order than one, so the two counts are recorded apart."""
import pytest

from test_dropan_transcripts import FIXTURE, load_script

pytestmark = pytest.mark.gpu


def test_gpu_runs_reproduce_the_recorded_transcripts():
    dt = load_script()
    expected = dt.load_fixture(FIXTURE, "gpu")
    assert len(expected) == 4 and all(e["status"] == 0 and all(e["files"].values()) for e in expected.values())
    assert all("Threshold DrainDen NoFirstOrd" in e["stdout"] and "Value for optimum that drop analysis selected" in e["stdout"] for e in expected.values())
    bad = dt.differences(expected, dt.collect("gpu"))
    assert not bad, "\n".join(bad)
