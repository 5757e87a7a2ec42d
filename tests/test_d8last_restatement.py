"""The C restatement of FlowDirCond, D8VDistToStrm and SlopeAveDown (tests/d8last_model.py) against the reference's outputs
(tests/golden/d8last_*.npz), bit for bit: the conditioned elevations, the two vertical-distance runs (the Threshold raster with the default
-thresh 1, the contributing-area raster with -thresh 40) and the three slope rasters (niter 1, 3 and 7).  CPU only."""
import numpy as np
import pytest

import d8last_model as M
from conftest import bits_equal, describe_diff

CASES = ("fourway_mask", "geographic", "holes", "plain", "rect_dxdy")
MISSING = np.float32(-3.4028235e38)   # MISSINGFLOAT: the nodata of the distance and slope rasters


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("d8last"))


def test_all_five_cases_have_a_fixture():
    assert tuple(M.golden_names()) == CASES


@pytest.mark.parametrize("name", CASES)
def test_flowdircond_equals_reference(restate, name):
    g = M.load_golden(name)
    out = restate.flowdircond(g["p"], g["z"], float(g["fel_nodata"]))
    assert bits_equal(out, g["zfdc"]), describe_diff(out, g["zfdc"], f"{name}: zfdc")


@pytest.mark.parametrize("name", CASES)
def test_vertical_distance_equals_reference(restate, name):
    g = M.load_golden(name)
    out = restate.vdist(g["p"], g["fel"], g["src"], 1, src_nodata=int(g["src_nodata"]))
    assert bits_equal(out, g["vdist_src"]), describe_diff(out, g["vdist_src"], f"{name}: -src src")
    out = restate.vdist(g["p"], g["fel"], g["ad8"], M.THRESH_AD8, src_nodata=int(g["ad8_nodata"]))
    assert bits_equal(out, g["vdist_ad8"]), describe_diff(out, g["vdist_ad8"], f"{name}: -src ad8 -thresh {M.THRESH_AD8}")


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_slopeavedown_equals_reference(restate, name, i):
    g = M.load_golden(name)
    dn = float(g["dn"][i])
    assert M.niter_of(dn, g["dxc"], g["dyc"]) == int(g["niter"][i]) == (1, 3, 7)[i]
    out = restate.slopeavedown(g["p"], g["fel"], dn, g["dxc"], g["dyc"], float(g["fel_nodata"]))
    assert bits_equal(out, g[f"slpd_{i}"]), describe_diff(out, g[f"slpd_{i}"], f"{name}: -dn {dn}")


def test_goldens_cover_the_quirks():
    """The fixtures exercise what the semantics single out: p == 0 cells, the 2-cell cycle, a stream cell without a direction, nodata fel under
    a valid direction - some of those cells with contributors, so that a cell acquires ed / dd in the first pass and hands them on from the
    second, and its nodata z enters a slope.  FlowDirCond lowered at least 3 % of all cells and left at least 50 % unchanged; each slope
    raster has a value on at least 50 % of all cells and the three distances give three different rasters; the vertical distance has a
    value on at least 40 % of all cells."""
    dx_, dy_ = (0, 1, 1, 0, -1, -1, -1, 0, 1), (0, 0, -1, -1, -1, 0, 1, 1, 1)
    for name in CASES:
        g = M.load_golden(name)
        p, src, fel, z = g["p"], g["src"], g["fel"], g["z"]
        ny, nx = p.shape
        stream = (src != g["src_nodata"]) & (src >= 1)
        assert np.any(p == 0), name
        assert np.any((p[:, :-1] == 1) & (p[:, 1:] == 5)), name
        assert np.any(stream & (p == M.P_NODATA)), name
        hole = (fel < -1e30) & (p >= 1) & (p <= 8)
        assert np.any(hole), name
        fed = False                                    # a nodata-fel cell with a valid code that some cell with a value drains into
        for y, x in zip(*np.nonzero(hole)):
            for k in range(1, 9):
                yn, xn = y - dy_[k], x - dx_[k]
                if 0 <= yn < ny and 0 <= xn < nx and p[yn, xn] == k and fel[yn, xn] > -1e30:
                    fed = True
        assert fed, name
        assert np.any(hole & (g["slpd_2"] != MISSING) & (g["slpd_2"] < -1e30)), name   # the nodata value entered a slope
        changed = g["zfdc"].view(np.uint32) != z.view(np.uint32)
        assert np.all(g["zfdc"][changed] < z[changed]), name
        assert 0.03 <= changed.mean() <= 0.5, (name, float(changed.mean()))
        assert np.array_equal(g["zfdc"][z < -1e30].view(np.uint32), z[z < -1e30].view(np.uint32)), name
        for i in range(3):
            assert np.mean(g[f"slpd_{i}"] != MISSING) >= 0.5, (name, i)
        assert not bits_equal(g["slpd_0"], g["slpd_1"]) and not bits_equal(g["slpd_1"], g["slpd_2"]) and not bits_equal(g["slpd_0"], g["slpd_2"]), name
        for key in ("vdist_src", "vdist_ad8"):
            assert np.mean(g[key] != MISSING) >= 0.4, (name, key)
            assert np.all(g[key][stream if key == "vdist_src" else (g["ad8"] >= M.THRESH_AD8)] == 0.0), name
        assert not bits_equal(g["vdist_src"], g["vdist_ad8"]), name
