"""The serial restatement of DropAnalysis (tests/dropan_model.py) against the reference's 1-rank outputs (tests/golden/dropan_*.npz), byte for byte: on one
rank the reference's queue order makes its float sums, and so its table, reproducible to the last digit.  The product's host formatting
(tdx_dropanalysis_table: the ladder's thresholds, the reference's float / double expressions, the optimum) is then held to the same bytes, fed the
restatement's float sums - no GPU.  The rasters of tests/pathological.py are held the same way: tests/golden/dropan_patho.npz has the reference's table and
console bytes for inputs that dropan_strips.patho_case derives again here.  CPU only."""
import numpy as np
import pytest

import dropan_model as M
import dropan_strips as S
import pathological as PG
import taudem_amd as T

RUNS = [(name, st) for name in M.CASES for st in (0, 1)]
NO_OPTIMUM = ("fourway_mask", 1)


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("dropan"))


@pytest.fixture(scope="module")
def runs(restate):
    """the restatement's run of every golden, made once"""
    out = {}
    for name, st in RUNS:
        g = M.load_golden(name)
        tmin, tmax, nt = g["par"]
        out[name, st] = restate.run(g["ad8"], g["p"], g["fel"], g["ad8"], g["cols"], g["rows"], g["dxc"], g["dyc"], tmin, tmax, int(nt), st)
    return out


def test_all_five_cases_have_a_fixture():
    import glob
    import os

    assert sorted(os.path.basename(f)[7:-4] for f in glob.glob(os.path.join(M.GOLDEN, "dropan_*.npz"))) == sorted(M.CASES + ("patho",))


@pytest.mark.parametrize("name,st", RUNS)
def test_table_equals_reference(runs, name, st):
    g = M.load_golden(name)
    assert runs[name, st]["table"] == M.text_of(g[f"table_{st}"])


@pytest.mark.parametrize("name,st", RUNS)
def test_console_lines_equal_reference(runs, name, st):
    """the header, one line per threshold (` - ` for undefined entries) and the optimum line, as the reference's stdout has them"""
    g = M.load_golden(name)
    ref = M.text_of(g[f"console_{st}"]).decode()
    assert runs[name, st]["console"].decode() in ref


@pytest.mark.parametrize("name,st", RUNS)
def test_product_table_equals_reference(runs, name, st):
    g = M.load_golden(name)
    r = runs[name, st]
    s = np.array([q["s"] for q in r["per"]], np.float32)
    table, console, opt = T.dropanalysis_table(r["thresh"], [q["n1"] for q in r["per"]], [q["n2"] for q in r["per"]], s[:, 0], s[:, 1], s[:, 2], s[:, 3],
                                               [q["length"] for q in r["per"]], r["total_area"])
    assert table.encode() == M.text_of(g[f"table_{st}"])
    assert console.encode() == r["console"]
    if (name, st) == NO_OPTIMUM:
        assert opt is None and table.endswith("Optimum Threshold Value: 0.000000\n")
    else:
        assert opt is not None and opt == r["optimum"] and f"{float(opt):f}" == table.strip().split(": ")[-1]   # (the table prints six decimals)


def test_exactly_one_run_has_no_optimum(runs):
    assert [k for k in RUNS if runs[k]["optimum"] is None] == [NO_OPTIMUM]
    rows, opt = M.parse_table(runs[NO_OPTIMUM]["table"])
    assert opt == 0.0 and len(rows) >= 6 and not np.any(np.abs(rows[:, 8]) < 2.0)


def test_goldens_cover_what_the_semantics_single_out(runs):
    """at least six rows per run, an optimum that is not the first row, no |t| within 0.01 of 2 (so that rounding cannot move the optimum), noise recorded"""
    later = 0
    for name, st in RUNS:
        g = M.load_golden(name)
        rows, opt = M.parse_table(M.text_of(g[f"table_{st}"]))
        assert len(rows) >= 6, (name, st)
        assert np.min(np.abs(np.abs(rows[:, 8]) - 2.0)) > 0.01, (name, st)
        assert g[f"noise_{st}"].shape == (5,) and np.all(g[f"noise_{st}"] < 1e-3), (name, st)
        later += (name, st) != NO_OPTIMUM and opt != rows[0, 0]
    assert later >= 1


def test_order_rule_is_not_strahler(restate):
    """inflow orders (1,1,2,2) in neighbour order give 2, (2,2,1,1) give 3 (src/DropAnalysis.cpp:113-166)"""
    import dropan_rasters as DR

    for orders, want in (((1, 1, 2, 2), 2), ((2, 2, 1, 1), 3)):
        p, fel, ssa, (jx, jy) = DR.junction(orders)
        q = restate.threshold(p, fel, ssa, 1.0, 1.0, 1.0)
        assert q["order"][jy, jx] == want


# ---- the rasters of tests/pathological.py ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def patho():
    import os

    return dict(np.load(os.path.join(M.GOLDEN, "dropan_patho.npz")))


def test_every_pathological_case_has_the_reference_table(patho):
    """the reference finished on all of them, the rasters without a single flow direction included"""
    assert sorted(k[6:-2] for k in patho if k.startswith("table_") and k.endswith("_0")) == sorted(PG.CASES)


@pytest.mark.parametrize("name", sorted(PG.CASES))
def test_pathological_table_and_console_equal_reference(restate, oracle, patho, name):
    c = S.patho_case(oracle, name)
    assert np.array_equal(c["cols"], patho[f"cols_{name}"]) and np.array_equal(c["rows"], patho[f"rows_{name}"]) and tuple(patho[f"par_{name}"]) == c["par"]
    for st in (0, 1):
        r = restate.run(c["ad8"], c["p"], c["fel"], c["ad8"], c["cols"], c["rows"], c["dx"], c["dy"], *c["par"], st)
        assert r["table"] == M.text_of(patho[f"table_{name}_{st}"]), (name, st)
        assert r["console"].decode() in M.text_of(patho[f"console_{name}_{st}"]).decode(), (name, st)
        s = np.array([q["s"] for q in r["per"]], np.float32)
        table, console, opt = T.dropanalysis_table(r["thresh"], [q["n1"] for q in r["per"]], [q["n2"] for q in r["per"]], s[:, 0], s[:, 1], s[:, 2], s[:, 3],
                                                   [q["length"] for q in r["per"]], r["total_area"])
        assert table.encode() == r["table"] and console.encode() == r["console"] and (opt is None) == (r["optimum"] is None), (name, st)
