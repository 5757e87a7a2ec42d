"""DropAnalysis on inputs that are nothing like a fractal surface (tests/pathological.py): planes, ramps, a spiral, single rows and columns, rasters without
data, NaN and Inf cells.  fel, p and ad8 are the CPU oracle's (dropan_strips.patho_case: ssa = ad8, a log ladder of five thresholds), the expected values the
serial restatement's, which tests/test_dropan_restatement.py holds to the reference's tables on these very inputs (tests/golden/dropan_patho.npz).  Each
case runs on one device (dropan_strips.check) and in three row strips of partition_rows - in as many strips as it has rows where it has fewer than
three - with the assertions of the random cuts (dropan_strips.assert_strips); both under the sweep verifier.  Counts and grids are exact; a sum or a
table column that is NaN or infinite is held to its class.

What the reference did on these inputs (tests/golden/make_golden_dropan.py; it finished on all 18, none is left out of the golden), log / arithmetic:
    nan_cells, +inf_cells   4 / 2 rows, optimum 166.321976 / none, min ||t| - 2| 0.8161 / 3.5378
    -inf_cells              4 / 2 rows, optimum 166.31752 / none,  min ||t| - 2| 0.8805 / 3.5378
    spiral                  1 / 1 row,  no optimum,                min ||t| - 2| 12.7216
    the other 14            no row, no optimum, no t: n1 = n2 = 0 at every threshold on the plane, the ramps and the checkerboard; the rasters of one or
                            two rows, all_nodata and one_data_cell have no cell with a direction (ladder 2 .. 2)
The restatement's drop lists are finite on all 18, so no sum here is NaN or infinite today; the class rule is pinned by tests/test_dropan_strips_model.py.
On an MI355X a case takes at most 0.2 s in either form; one_row in strips takes 4 s (a group of one rank on a device of its own sets up RCCL)."""
import pytest

import dropan_model as M
import dropan_strips as S
import pathological as PG
from taudem_amd.distributed import partition_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("dropan"))


@pytest.fixture(scope="module")
def cases(oracle):
    """the derived inputs, made once per case and shared by the two tests"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = S.patho_case(oracle, name)
        return made[name]
    return get


@pytest.mark.parametrize("name", sorted(PG.CASES))
def test_one_device_on_pathological_input(ctx, restate, cases, monkeypatch, name):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    c = cases(name)
    S.check(ctx, restate, c["ad8"], c["p"], c["fel"], c["ad8"], c["cols"], c["rows"], c["dx"], c["dy"], c["par"], 0, name, grid_th=1, nan_aware=True)


@pytest.mark.parametrize("name", sorted(PG.CASES))
def test_three_strips_on_pathological_input(restate, cases, monkeypatch, name):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    c = cases(name)
    ny = c["p"].shape[0]
    parts = partition_rows(ny, min(3, ny))
    ref = restate.run(c["ad8"], c["p"], c["fel"], c["ad8"], c["cols"], c["rows"], c["dx"], c["dy"], *c["par"], 0)
    results, comb = S.in_strips((c["ad8"], c["p"], c["fel"], c["ad8"]), parts, c["dx"], c["dy"], (c["cols"], c["rows"]), c["par"], 0, 1)
    S.assert_strips(results, comb, ref, c["p"], c["fel"], parts, c["dx"], c["dy"], 1, f"{name} in {len(parts)} strips", nan_aware=True)
