"""The restatements held to the REAL reference on inputs that are nothing like a fractal surface (tests/golden/patho_*.npz, reduced
versions of tests/pathological.py's rasters: a plane, ramps, a checkerboard of pits, a spiral channel, 1 x N / N x 1 / 2 x N rasters,
all-nodata, one data cell, NaN and +-Inf cells).  The five fractal goldens pin them on terrain-like rasters only; the GPU tests on the
pathological rasters (tests/test_gpu_pathological.py, tests/test_gpu_pathological_downstream.py) trust them at full size.  Every tool
from PitRemove to the downstream tools, bit for bit; GageWatershed's -id text byte for byte."""
import numpy as np
import pytest

import downstream as D
import patho_fixture as F
from conftest import bits_equal, describe_diff

NAMES = F.names()


@pytest.fixture(scope="module")
def R(tmp_path_factory, oracle):
    return D.Restate(tmp_path_factory.mktemp("patho"), oracle)


def test_fixtures_cover_the_cases():
    assert set(NAMES) >= {"plane", "ramp_shallow", "ramp_diag", "checkerboard_pits", "spiral", "one_row", "one_column", "two_rows", "all_nodata",
                          "one_data_cell", "nan_cells", "+inf_cells", "-inf_cells"}
    # every (stat, kind) of DinfDistDown and of DinfDistUp, and every variant, comes up in some fixture
    keys = set().union(*(F.load(n).keys() for n in NAMES))
    for st, kd in D.MODES:
        assert any(k.startswith(f"dd_{st}_{kd}") for k in keys), (st, kd)
        assert any(k.startswith(f"du_{st}_{kd}") for k in keys), (st, kd)
    for sfx in ("_nc", "_wg"):
        assert any(k.startswith("dd_") and k.endswith(sfx) for k in keys), sfx
    for sfx in ("_nc", "_wg", "_t"):
        assert any(k.startswith("du_") and k.endswith(sfx) for k in keys), sfx


@pytest.mark.parametrize("name", NAMES)
def test_upstream_restatement_matches_reference(name, oracle):
    g = F.load(name)
    dx, dy = F.DX, F.DY
    fel = oracle.pitremove(g["dem"], -9999.0)
    assert bits_equal(fel, g["fel"]), describe_diff(fel, g["fel"], f"{name}: fel")
    p, sd8, _ = oracle.d8flowdir(g["fel"], -3.0e38, dx, dy)
    assert bits_equal(p, g["p"]), describe_diff(p, g["p"], f"{name}: p")
    assert bits_equal(sd8, g["sd8"]), describe_diff(sd8, g["sd8"], f"{name}: sd8")
    ang, slp, _ = oracle.dinfflowdir(g["fel"], -3.0e38, dx, dy)
    assert bits_equal(ang, g["ang"]), describe_diff(ang, g["ang"], f"{name}: ang")
    assert bits_equal(slp, g["slp"]), describe_diff(slp, g["slp"], f"{name}: slp")
    for cc, key in ((True, "ad8"), (False, "ad8_nc")):
        a = oracle.aread8(g["p"], -32768, contcheck=cc)
        assert bits_equal(a, g[key]), describe_diff(a, g[key], f"{name}: {key}")
    for cc, key in ((True, "sca"), (False, "sca_nc")):
        a = oracle.areadinf(g["ang"], D.ANG_ND, dx, dy, contcheck=cc)
        assert bits_equal(a, g[key]), describe_diff(a, g[key], f"{name}: {key}")


@pytest.mark.parametrize("name", NAMES)
def test_downstream_restatements_match_reference(name, R):
    g = F.load(name)
    exp = F.expected(g)
    got = F.restated(R, g)
    assert set(got) == set(exp)
    bad = D.compare(got, exp, name)
    assert not bad, "\n".join(bad)
