"""The restatements held to the REAL reference on inputs that are nothing like a fractal surface (tests/golden/patho_*.npz, reduced
versions of tests/pathological.py's rasters: a plane, ramps, a checkerboard of pits, a spiral channel, 1 x N / N x 1 / 2 x N rasters,
all-nodata, one data cell, NaN and +-Inf cells).  The five fractal goldens pin them on terrain-like rasters only; the GPU tests on the
pathological rasters (tests/test_gpu_pathological.py, tests/test_gpu_pathological_downstream.py) trust them at full size.  Every tool
from PitRemove to the downstream tools, bit for bit; GageWatershed's -id text byte for byte.  The five late sweep tools have fixtures of
their own (patholate_*.npz): qrl, zfdc, vd* and slpd* bit for bit; rz / dfs under the rule of tests/test_aval_restatement.py - bit for bit
where the host's libc is the one that made the fixtures (the reference calls its float atan), and under aval_model.compare_aval anywhere."""
import numpy as np
import pytest

import aval_model
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


def test_late_fixtures_cover_the_cases():
    assert F.late_names() == NAMES
    assert {n for n in NAMES if str(F.load_late(n)[0]["direct"]) == "single"} == set(D.LATE_DIRECT) & set(NAMES)


@pytest.mark.parametrize("name", F.late_names())
def test_late_restatements_match_reference(name, R, oracle):
    g, inp = F.load_late(name)
    i = int(g["index"])
    ang_a = oracle.dinfflowdir(inp["fel"], D.FEL_ND, *D.PYTH)[0]
    assert bits_equal(ang_a, g["in_ang_a"]), describe_diff(ang_a, g["in_ang_a"], f"{name}: the angles on 30 x 40 cells")
    got = D.reference_late(R, inp, F.DX, F.DY, i)
    exp = F.expected_late(g, R, inp)
    assert set(got) == set(exp)
    bad = D.compare_late(got, exp, name)        # everything but rz / dfs bit for bit; rz / dfs under the tolerant rule
    if str(g["libc"]) == aval_model.libc_tag():
        bad += [describe_diff(got[k], exp[k], f"{name}: {k} (same libc: bit for bit)") for k in exp if k[:3] in ("rz_", "dfs") and not bits_equal(got[k], exp[k])]
    assert not bad, "\n".join(bad)
    # the chosen sources are the ones extras_late chooses again, and every other new input is drawn again with the same bits
    again = D.extras_late({k: v for k, v in F.inputs(F.load(name)).items()} | {"ang_a": g["in_ang_a"]}, 40 + i, R, F.DX, F.DY, i,
                          direct=D.LATE_DIRECT.get(name, "scattered"))
    for k in g:
        if k.startswith("in_"):
            assert bits_equal(again[k[3:]], g[k]), k
