"""The SinmapSI restatement (tests/sinmap/sinmap_restate.cpp) against what the real tool wrote (tests/golden/sinmap_*.npz, made by
tests/golden/make_golden_sinmap.py): the "double" variant bit for bit, NaN patterns included; the "long" and "fast" variants on the same path in every
cell, with the same sat, and within the stored E_abs of it.  No GPU is needed."""
import numpy as np
import pytest

import sinmap_model as M


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("sinmap_restate"))


def _same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _runs(name):
    return M.patho_runs() if name == "patho" else M.golden_runs(name)


@pytest.mark.parametrize("case", M.CASES + ("patho",))
def test_restatement_equals_the_reference(restate, case):
    gold, meta = M.load_golden(case)
    runs = _runs(case)
    assert sorted(gold) == sorted(k for k, _ in runs)
    for key, r in runs:
        si, sat, code = restate.run("double", r)
        g = gold[key]
        assert _same_bits(si, g["si"]) and _same_bits(sat, g["sat"]) and np.array_equal(code, g["code"]), (case, key)
        for name in ("long", "fast"):
            osi, osat, ocode = restate.run(name, r)
            assert np.array_equal(ocode, code) and _same_bits(osat, sat), (case, key, name)
            fin = np.isfinite(si)
            assert np.array_equal(np.isfinite(osi), fin)
            assert np.all(np.abs(osi[fin].astype(np.float64) - si[fin].astype(np.float64)) <= meta["E_abs"]), (case, key, name)
    assert 0.0 <= meta["E_abs"] < 1e-6 and meta["ulp_spread"] <= 1.0


def test_every_path_code_occurs_in_the_committed_set():
    seen = set()
    for case in M.CASES + ("patho",):
        for g in M.load_golden(case)[0].values():
            seen |= set(np.unique(g["code"]).tolist())
    assert seen == set(M.ALL_CODES)


def test_runs_without_recharge_write_only_where_scamax_is_not_zero():
    for case in M.CASES:
        gold, _ = M.load_golden(case)
        runs = dict(M.golden_runs(case))
        assert np.all(gold["r0_noroads"]["si"] == -1.0) and np.all(gold["r0_noroads"]["sat"] == -1.0) and (gold["r0_noroads"]["code"] == M.NOT_WRITTEN).any()
        w = gold["r0_roads"]["code"] > M.NOT_WRITTEN
        assert w.any() and np.all(runs["r0_roads"]["scamax"][w] != 0)


def test_duplicate_hex_and_octal_ids_and_a_listed_nodata_value():
    for case in M.CASES:
        gold, _ = M.load_golden(case)
        assert _same_bits(gold["calpar_variant"]["si"], gold["noroads"]["si"]) and _same_bits(gold["calpar_variant"]["sat"], gold["noroads"]["sat"])
        band2 = dict(M.golden_runs(case))["posnd"]["cal"] == 2
        assert band2.sum() > 1000 and np.all(gold["posnd"]["code"][band2] == M.NODATA) and (gold["noroads"]["code"][band2] != M.NODATA).any()
