"""The assertions of the DropAnalysis strip tests (dropan_strips.assert_strips) on the CPU, fed the restatement's own per-strip split in place of the device's
results: they pass on the split as it is and fail on each of five planted errors, so that they cannot silently pass everything.  Also the conditions
tests/test_gpu_dropan_strips.py asks of its random inputs, from the restatement alone, for every seed and step type.  CPU only."""
import copy

import numpy as np
import pytest

import dropan_model as M
import dropan_strips as S
import peuker_model as PM

SEED, STEPTYPE = 1, 0      # four strips, `wild` per-row cell sizes, Peuker-Douglas weighted ssa


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("dropan"))


@pytest.fixture(scope="module")
def peuker(tmp_path_factory):
    return PM.compile(tmp_path_factory.mktemp("peuker"))


@pytest.fixture(scope="module")
def case(oracle, restate, peuker):
    c = S.random_case(oracle, peuker, SEED)
    par = S.ladder_of(c["ssa"], STEPTYPE)
    c["ref"] = restate.run(c["ad8"], c["p"], c["fel"], c["ssa"], c["cols"], c["rows"], c["dx"], c["dy"], *par, STEPTYPE)
    return c


def _split(c, **kw):
    return S.expected_split(c["ref"], c["p"], c["fel"], c["ad8"], c["ssa"], (c["cols"], c["rows"]), c["parts"], c["dx"], c["dy"], c["grid_th"], **kw)


def _assert(c, results, comb=None):
    comb = S.combine(results, c["parts"], c["dx"], c["dy"]) if comb is None else comb
    S.assert_strips(results, comb, c["ref"], c["p"], c["fel"], c["parts"], c["dx"], c["dy"], c["grid_th"], "planted")


def test_the_split_of_the_restatement_passes(case):
    assert len(case["parts"]) == 4 and not np.isscalar(case["dx"]) and all(int(r[1][0]) > 0 and int(r[2][0]) > 0 for r in _split(case))
    _assert(case, _split(case))


def test_a_dropped_n1_fails(case):
    results = _split(case)
    comb = S.combine(results, case["parts"], case["dx"], case["dy"])
    comb["n1"] = comb["n1"] - results[2][1]                     # one strip's n1 left out of the combination
    with pytest.raises(AssertionError, match="n1, n2 of threshold 0"):
        _assert(case, results, comb)


def test_a_drop_counted_by_the_wrong_strip_fails(case):
    results = [list(r) for r in _split(case)]
    results[1][1], results[2][1] = results[1][1] + results[2][1], np.zeros_like(results[2][1])   # the totals are right
    with pytest.raises(AssertionError, match=r"strip 1 \(rows .*n1, n2"):
        _assert(case, results)


def test_cell_sizes_shifted_by_one_row_fail(case):
    with pytest.raises(AssertionError, match="length of threshold 0"):
        _assert(case, _split(case, shift_rows=1))
    with pytest.raises(AssertionError, match="length of threshold 0"):
        _assert(case, _split(case, shift_rows=-1))


def test_swapped_order_rows_fail(case):
    results = [list(r) for r in _split(case)]
    results[0][6], results[1][6] = results[1][6], results[0][6]
    with pytest.raises(AssertionError, match="order grid"):
        _assert(case, results)


def test_sums_added_twice_fail(case):
    results = _split(case)
    comb = S.combine(results, case["parts"], case["dx"], case["dy"])
    twice = copy.deepcopy(comb)
    twice["sums"] = comb["sums"] + results[3][3]
    with pytest.raises(AssertionError, match="sum 0 of threshold 0"):
        _assert(case, results, twice)


@pytest.mark.parametrize("seed", S.SEEDS)
def test_inputs_of_the_random_cuts_meet_their_conditions(oracle, restate, peuker, seed):
    """at least 4 written rows with n2 > 0 in the first, no |t| within 0.01 of 2, a junction on a row next to a cut; one seed has a strip of one owned row,
    one has cuts directly under row 0 and directly above the last row"""
    c = S.random_case(oracle, peuker, seed)
    sizes = [y1 - y0 for y0, y1 in c["parts"]]
    assert 2 <= len(sizes) <= 8 and min(sizes) >= 1
    assert seed != S.ONE_ROW_SEED or 1 in sizes
    assert seed != S.EDGE_SEED or (c["parts"][0] == (0, 1) and c["parts"][-1] == (c["ny"] - 1, c["ny"]))
    for st in (0, 1):
        ref = restate.run(c["ad8"], c["p"], c["fel"], c["ssa"], c["cols"], c["rows"], c["dx"], c["dy"], *S.ladder_of(c["ssa"], st), st)
        nrows, n2_first, margin, on_cut = S.input_conditions(ref, c["p"], c["parts"])
        print(f"seed {seed} steptype {st}: {c['ny']} x {c['nx']} in {len(sizes)} strips, {nrows} rows, n2 {n2_first}, min ||t| - 2| {margin:.4f}, {on_cut} junctions on cut rows")
        assert nrows >= 4 and n2_first > 0 and margin > 0.01 and on_cut >= 1


def test_sums_with_nan_or_inf_are_held_to_their_class():
    """no raster of the suite makes such a sum today; the rule is pinned here"""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    d = np.array([1.5, 2.5], np.float32)
    assert S.exact_sums(d, d[:1]) == M.sums_from_drops(d, d[:1]) and S.abs_sums(-d, d) == M.abs_sums_from_drops(-d, d)
    assert np.isnan(S.exact_sums(np.array([inf, -inf], np.float32), d)[0]) and np.isnan(S.exact_sums(np.array([1.0, nan], np.float32), d)[1])
    assert S.exact_sums(np.array([-inf, 1.0], np.float32), d)[:2] == [-np.inf, np.inf]
    assert S.sum_within(np.nan, np.nan, np.nan, 2) and S.sum_within(np.inf, np.inf, np.inf, 2)
    assert not S.sum_within(1.0, np.nan, np.nan, 2) and not S.sum_within(-np.inf, np.inf, np.inf, 2) and not S.sum_within(np.nan, 4.0, 4.0, 2)
    assert S.sum_within(4.0, 4.0, 4.0, 2) and not S.sum_within(4.0 + 1e-12, 4.0, 4.0, 2)
    head = "Threshold, DrainDen, NoFirstOrd,NoHighOrd, MeanDFirstOrd, MeanDHighOrd, StdDevFirstOrd, StdDevHighOrd, T\n"
    row = "2.000000, 1.0e-03, 5, 4, {}, 1.000000, 2.000000, 1.000000, {}\n"
    tail = "Optimum Threshold Value: 0.000000\n"
    a, b, c = ((head + row.format(*v) + tail).encode() for v in (("nan", "-nan"), ("-nan", "nan"), ("3.000000", "nan")))
    assert S.same_tables(a, b, True) and S.same_tables(a, c) and not S.same_tables(a, c, True)
