"""The C restatement of RetLimFlow and DinfAvalanche (tests/aval_model.py) against the reference's rasters (tests/golden/aval_*.npz): qrl bit for
bit always; rz / dfs bit for bit when the host libc is the one that made the fixtures (the reference calls its float atan), otherwise under
the tolerant rule the GPU tests use.  CPU only."""
import numpy as np
import pytest

import aval_model as M
from conftest import bits_equal, describe_diff


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("aval"))


@pytest.mark.parametrize("name", M.golden_names())
def test_retlimflow_restatement_equals_reference(restate, name):
    g = M.load_golden(name)
    out = restate.retlimflow(g["ang"], g["wg"], g["rc"], dxc=g["dxc"], dyc=g["dyc"])
    assert bits_equal(out, g["qrl"]), describe_diff(out, g["qrl"], f"{name}: qrl")


@pytest.mark.parametrize("name", M.golden_names())
def test_avalanche_restatement_equals_reference_bit_for_bit(restate, name):
    g = M.load_golden(name)
    if str(g["libc"]) != M.libc_tag():
        pytest.skip(f"the fixture was made with libc {g['libc']}, this host has {M.libc_tag()}: atanf may round differently (the tolerant test covers it)")
    bad = []
    for sfx, direct, ta in M.variants():
        rz, dfs, _ = M.run_aval(restate, g, direct, ta)
        for out, key in ((rz, "rz" + sfx), (dfs, "dfs" + sfx)):
            if not bits_equal(out, g[key]):
                bad.append(describe_diff(out, g[key], f"{name}: {key}"))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", M.golden_names())
def test_avalanche_restatement_equals_reference_within_the_tolerance(restate, name):
    """The rule of the GPU tests, with the restatement in the GPU's place: same cells, same dfs, rz within TOL_ULPS outside the tainted cells, and
    at most 1 % of the runout tainted."""
    g = M.load_golden(name)
    bad = []
    for sfx, direct, ta in M.variants():
        rz, dfs, taint = M.run_aval(restate, g, direct, ta)
        bad += M.compare_aval(rz, dfs, g["rz" + sfx], g["dfs" + sfx], taint, f"{name}{sfx}")
    assert not bad, "\n".join(bad)


def test_goldens_cover_the_quirks(restate):
    """The fixtures exercise what the semantics single out."""
    for name in M.golden_names():
        g = M.load_golden(name)
        ang, fel, wg, rc, ass, qrl = (g[k] for k in ("ang", "fel", "wg", "rc", "ass", "qrl"))
        ang_nd = ang < -1e30
        inner = np.zeros(ang_nd.shape, bool)
        inner[1:-1, 1:-1] = True
        assert np.any(ang_nd & inner) and np.any((ang == -1.0) & inner), name     # interior cells without an angle / without a direction
        # a nodata wg cell under a valid angle, and cells downstream of such cells that have no value although all their own inputs are data
        own_nd = (wg == M.WG_NODATA) | (rc == M.RC_NODATA)
        assert np.any((wg == M.WG_NODATA) & ~ang_nd) and np.any((rc == M.RC_NODATA) & ~ang_nd), name
        assert np.any((qrl < -1e30) & ~ang_nd & ~own_nd), name
        assert np.any((qrl == 0.0) & (rc > wg) & ~own_nd), name                    # the clamp
        alpha = M.DEFAULT[1]
        rzp, rzd, dfp, dfd = g["rz_path"], g["rz_direct"], g["dfs_path"], g["dfs_direct"]
        src = (ass > 0) & (fel > -1e30) & ~ang_nd
        assert np.any(src & (rzp > np.float32(alpha))), name                       # a source overridden by a steeper one above it
        assert np.any(src & (rzp == np.float32(alpha)) & (dfp == 0.0)), name       # and one that kept itself
        no_thresh, _, _ = restate.dinfavalanche(ang, fel, ass, thresh=0.0, alpha=alpha, dxc=g["dxc"], dyc=g["dyc"])
        assert not bits_equal(no_thresh, rzp), name                                # the threshold removes contributors
        # path and direct pick different sources somewhere: the source elevation fel + tan(rz) * dfs differs by metres
        both = (rzp > -1e30) & (rzd > -1e30) & (dfp > 0) & (dfd > 0)
        zs = lambda rz, d: fel.astype(np.float64) + np.tan(np.radians(rz.astype(np.float64))) * d  # noqa: E731
        assert np.any(both & (np.abs(zs(rzp, dfp) - zs(rzd, dfd)) > 1.0)), name
        # a cell without an elevation under a valid angle, inside a runout: it has no value, its neighbours have
        fel_nd = (fel < -1e30) & ~ang_nd
        has = rzp > -1e30
        near = np.zeros_like(has)
        near[1:-1, 1:-1] = sum(has[1 + dj:has.shape[0] - 1 + dj, 1 + di:has.shape[1] - 1 + di] for dj in (-1, 0, 1) for di in (-1, 0, 1) if (dj, di) != (0, 0)) >= 2
        assert np.any(fel_nd & near) and not np.any(fel_nd & has), name
        assert not bits_equal(g["rz_path_o"], rzp) and not bits_equal(rzd, rzp), name
