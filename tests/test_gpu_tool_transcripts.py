"""Every command-line tool with --gpus 1 and --gpus 3, every optional branch, reproduces tests/golden/tool_transcripts.json entry
for entry: exit status, stdout and stderr (times blanked) and the SHA-256 of every output file; so does every tool's statistics
line (TAUDEM_AMD_STATS=1, one GPU; device time, rate and round count blanked).  The fixture is
scripts/tool_transcripts.py --record on a build of commit 1e7abfb, the last one before the file-level tool functions moved
onto one frame."""
import pytest

from test_tool_transcripts import FIXTURE, load_script

pytestmark = pytest.mark.gpu


def test_gpu_runs_reproduce_the_recorded_transcripts():
    tt = load_script()
    expected = tt.load_fixture(FIXTURE, "gpu")
    assert {rid.split("/")[2] for rid in expected} == set(tt.TOOLS)             # all 22 tools ...
    assert {rid.split("/")[0] for rid in expected} == {"gpu1", "gpu3"}         # ... on one GPU and on three strips
    assert all(e["status"] == 0 and all(e["files"].values()) for e in expected.values())
    stats = {rid.split("/")[2]: e["stderr"] for rid, e in expected.items() if rid.split("/")[1] == "stats"}
    assert set(stats) == set(tt.TOOLS)
    assert [t for t in tt.TOOLS if f'{{"tool": "{t}", ' not in stats[t]] == ["threshold"]   # the one tool without a statistics line
    bad = tt.differences(expected, tt.collect("gpu"))
    assert not bad, "\n".join(bad)
