"""The C restatement of D8HDistToStrm and GageWatershed (tests/d8rev_model.py) against the reference's outputs (tests/golden/d8rev_*.npz):
the distance rasters bit for bit (the Threshold raster with the default -thresh 1, and the contributing-area raster with -thresh 40), the
gauge raster exactly and the -id file byte for byte.  CPU only."""
import numpy as np
import pytest

import d8rev_model as M
from conftest import bits_equal, describe_diff


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("d8rev"))


@pytest.mark.parametrize("name", M.golden_names())
def test_distance_equals_reference(restate, name):
    g = M.load_golden(name)
    out = restate.dist(g["p"], g["src"], 1, g["dxc"], g["dyc"], src_nodata=int(g["src_nodata"]))
    assert bits_equal(out, g["dist_src"]), describe_diff(out, g["dist_src"], f"{name}: -src src")
    out = restate.dist(g["p"], g["ad8"], M.THRESH_AD8, g["dxc"], g["dyc"], src_nodata=int(g["ad8_nodata"]))
    assert bits_equal(out, g["dist_ad8"]), describe_diff(out, g["dist_ad8"], f"{name}: -src ad8 -thresh {M.THRESH_AD8}")


@pytest.mark.parametrize("name", M.golden_names())
def test_gage_watershed_equals_reference(restate, name):
    g = M.load_golden(name)
    gw, text = restate.gage(g["p"], g["cols"], g["rows"], g["ids"])
    assert np.array_equal(gw, g["gw"]), f"{name}: {int(np.sum(gw != g['gw']))} gauge labels differ"
    assert text == str(g["id_text"])


def test_goldens_cover_the_quirks():
    """The fixtures exercise what the semantics single out: p == 0 cells, stream cells without a direction (sources all the same), a
    cycle, src nodata holes, a gauge draining into another gauge, an outlet off the raster and two on one cell."""
    for name in M.golden_names():
        g = M.load_golden(name)
        p, src, d = g["p"], g["src"], g["dist_src"]
        stream = (src != g["src_nodata"]) & (src >= 1)
        assert np.any(p == 0), name
        assert np.all(d[stream] == 0.0) and np.any(stream & (p == M.P_NODATA)), name
        assert np.any((p[:, :-1] == 1) & (p[:, 1:] == 5)), name
        assert np.any(src == g["src_nodata"]), name
        assert not bits_equal(g["dist_ad8"], d), name
        lines = str(g["id_text"]).splitlines()
        assert lines[0] == "id iddown" and len(lines) - 1 == len(g["ids"]) - 2, name   # one off the raster, one on a taken cell
        assert any(int(line.split()[1]) in set(g["ids"].tolist()) for line in lines[1:]), name
        assert np.sum(np.isin(g["gw"], g["ids"])) > 0.05 * g["gw"].size, name
