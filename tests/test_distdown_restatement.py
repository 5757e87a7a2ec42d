"""The C restatement of DinfDistDown (tests/distdown_model.py) against the reference's rasters (tests/golden/distdown_*.npz), bit for
bit: every case, every -m combination, with and without the contamination check, with weights.  CPU only."""
import numpy as np
import pytest

import distdown_model as M
from conftest import bits_equal, describe_diff


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("distdown"))


@pytest.mark.parametrize("name", M.golden_names())
def test_restatement_equals_reference(restate, name):
    g = M.load_golden(name)
    bad = []
    for stat, kind, sfx in M.variants():
        out = restate(g["ang"], g["src"], g["fel"], stat=stat, kind=kind, weights=g["wg"] if sfx == "_wg" else None, contcheck=sfx != "_nc",
                      dxc=g["dxc"], dyc=g["dyc"])
        ref = g[f"dd_{stat}_{kind}{sfx}"]
        if not bits_equal(out, ref):
            bad.append(describe_diff(out, ref, f"{stat} {kind}{sfx}"))
    assert not bad, "\n".join(bad)


def test_goldens_cover_the_quirks():
    """The fixtures exercise what the semantics single out: a stream cell without an angle, nodata src and elevation cells, nodata
    weights, contamination that -nc lifts."""
    for name in M.golden_names():
        g = M.load_golden(name)
        ang_nd = np.abs(g["ang"] - np.float32(M.ANG_NODATA)) < 1e-5
        assert np.any((g["src"] >= 1) & ang_nd), name
        assert np.any(g["src"] == g["src_nodata"]), name
        assert np.any((g["fel"] < -1e30) & ~ang_nd), name
        assert np.any(g["wg"] == -9999.0), name
        assert np.sum(g["dd_ave_v_nc"] > -1e30) > np.sum(g["dd_ave_v"] > -1e30), name
        assert not bits_equal(g["dd_ave_h_wg"], g["dd_ave_h"]), name
        assert bits_equal(g["dd_ave_v_wg"], g["dd_ave_v"]), name   # v ignores the weights
