"""The PeukerDouglas restatement (tests/peuker/peuker_restate.cpp: the reference's sequential scan) against what the real tool wrote
(tests/golden/peuker_*.npz, made by tests/golden/make_golden_peuker.py), exactly.  No GPU is needed."""
import numpy as np
import pytest

import peuker_model as M


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("peuker_restate"))


@pytest.mark.parametrize("case", M.CASES)
def test_restatement_equals_the_reference_on_the_cases(restate, case):
    gold = M.load_golden(case)
    runs = M.golden_runs(case)
    assert sorted(gold) == sorted(k for k, *_ in runs)
    for key, z, nd, w in runs:
        ss = restate.run(z, nd, w)
        assert ss.dtype == np.int16 and np.array_equal(ss, gold[key]), (case, key, int(np.sum(ss != gold[key])))
    # both values are well represented, and an all-zero weight set flags nothing (0 / 0)
    assert 0.05 < gold["fel_default"].mean() < 0.5 and not gold["dem_par4"].any()


def test_positive_nodata_changes_the_result_next_to_holes():
    g = M.load_golden("fourway_mask")
    assert not np.array_equal(g["fel_default"], g["fel_pos9999"])


def test_restatement_equals_the_reference_on_the_pathological_rasters(restate):
    gold = M.load_golden("patho")
    inputs = M.patho_inputs()
    assert sorted(gold) == sorted(n for n, _ in inputs)
    for name, z in inputs:
        ss = restate.run(z, -9999.0, M.DEFAULT)
        assert np.array_equal(ss, gold[name]), (name, int(np.sum(ss != gold[name])))


def test_smoothed_grid_copies_rim_and_nodata(restate):
    z = M.golden_runs("holes")[0][1]
    _, sm = restate.run(z, M.FEL_NODATA, M.DEFAULT, smoothed=True)
    rim = np.ones(z.shape, bool)
    rim[1:-1, 1:-1] = False
    keep = rim | (z == M.FEL_NODATA)
    assert np.array_equal(sm[keep], z[keep]) and not np.array_equal(sm[~keep], z[~keep])
