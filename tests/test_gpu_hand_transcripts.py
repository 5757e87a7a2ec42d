"""bin/catchhydrogeo and bin/inundepth with --gpus 1 and --gpus 2 (InunDepth also with -mask) reproduce tests/golden/tool_transcripts_hand.json:
exit status, stdout and stderr (times blanked) and the SHA-256 of the table, the depth raster and the depth CSV.  The fixture is
scripts/hand_transcripts.py --record on the build that introduced the two tools."""
import pytest

from test_hand_transcripts import FIXTURE, load_script

pytestmark = pytest.mark.gpu


def test_gpu_runs_reproduce_the_recorded_transcripts():
    ht = load_script()
    expected = ht.load_fixture(FIXTURE, "gpu")
    assert len(expected) == 5 and all(e["status"] == 0 and all(e["files"].values()) for e in expected.values())
    assert expected["gpu1/plain/inundepth/depth"]["files"]["map.tif"] == expected["gpu2/plain/inundepth/depth"]["files"]["map.tif"]
    bad = ht.differences(expected, ht.collect("gpu"))
    assert not bad, "\n".join(bad)
