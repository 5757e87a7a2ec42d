"""The C restatement of DinfDistUp (tests/distup_model.py) against the reference's rasters (tests/golden/distup_*.npz), bit for bit: every
case, every -m combination, with and without the contamination check, with weights, with -thresh.  CPU only."""
import numpy as np
import pytest

import distup_model as M
from conftest import bits_equal, describe_diff


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("distup"))


@pytest.mark.parametrize("name", M.golden_names())
def test_restatement_equals_reference(restate, name):
    g = M.load_golden(name)
    bad = []
    for stat, kind, sfx in M.variants():
        out = M.run(restate, g, stat, kind, sfx)
        ref = g[f"du_{stat}_{kind}{sfx}"]
        if not bits_equal(out, ref):
            bad.append(describe_diff(out, ref, f"{stat} {kind}{sfx}"))
    assert not bad, "\n".join(bad)


def test_goldens_cover_the_quirks():
    """The fixtures exercise what the semantics single out: `max h` starting from 0, v on a nodata own elevation, a contributor the
    threshold removes, contamination that -nc lifts, weights that change h but not v, interior cells without an angle."""
    for name in M.golden_names():
        g = M.load_golden(name)
        ang_nd = g["ang"] < -1e30
        fel_nd = g["fel"] < -1e30
        inner = np.zeros(ang_nd.shape, bool)
        inner[1:-1, 1:-1] = True
        assert np.any(ang_nd & inner), name
        assert np.any(fel_nd & ~ang_nd), name
        assert np.any(g["wg"] == -9999.0), name
        # max h starts from 0, min h from the first contributor: with negative weights some cell has only negative candidates
        mh, nh = g["du_max_h_wg"], g["du_min_h_wg"]
        assert np.all(mh[mh > -1e30] >= 0), name
        assert np.any((mh == 0) & (nh < 0) & (nh > -1e30)), name
        # v has no own-elevation test: somewhere a cell with a nodata elevation has a (huge) value, where p and s have nodata
        v = g["du_ave_v_nc"]
        assert np.any(fel_nd & ~ang_nd & (v > 1e37)), name
        assert not np.any(fel_nd & (g["du_ave_s_nc"] > -1e30)), name
        assert not np.any(fel_nd & (g["du_ave_p_nc"] > -1e30)), name
        # the threshold removes contributors
        assert not bits_equal(g["du_ave_h_t"], g["du_ave_h"]), name
        assert not bits_equal(g["du_max_v_t"], g["du_max_v"]), name
        assert np.sum(g["du_ave_h_nc"] > -1e30) > np.sum(g["du_ave_h"] > -1e30), name
        assert not bits_equal(g["du_ave_h_wg"], g["du_ave_h"]), name
        assert bits_equal(g["du_ave_v_wg"], g["du_ave_v"]), name   # v ignores the weights

