"""The C restatement of CatchHydroGeo and InunDepth (tests/hand_model.py) against the reference's outputs (tests/golden/hand_*.npz), byte for
byte: the hydraulic property table, the depth raster with and without -mask and the depth CSV.  The serial scan order of the reference on
one rank makes the text files reproducible to the last digit.  CPU only."""
import numpy as np
import pytest

import hand_model as M
from conftest import bits_equal, describe_diff

CASES = ("fourway_mask", "geographic", "holes", "plain", "rect_dxdy")


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("hand"))


def _write(tmp_path, g, key, name):
    p = tmp_path / name
    p.write_bytes(M.text_of(g[key]))
    return str(p)


def test_all_five_cases_have_a_fixture():
    assert tuple(M.golden_names()) == CASES


@pytest.mark.parametrize("name", CASES)
def test_table_equals_reference(restate, tmp_path, name):
    g = M.load_golden(name)
    out = str(tmp_path / "table.txt")
    restate.chg_tool(g["hand"], g["catch"], g["slp"], g["dxc"], g["dyc"], _write(tmp_path, g, "list_csv", "list.csv"), _write(tmp_path, g, "stages_txt", "stages.txt"), out)
    assert open(out, "rb").read() == M.text_of(g["table_txt"])


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("masked", [False, True])
def test_map_and_depths_equal_reference(restate, tmp_path, name, masked):
    g = M.load_golden(name)
    ids, flow, depth, carea = restate.inun_depths(_write(tmp_path, g, "fc_csv", "fc.csv"), _write(tmp_path, g, "table_txt", "table.txt"))
    m = restate.inun_map(g["hand"], g["catch"], ids, depth, g["mask"] if masked else None)
    want = g["map_mask" if masked else "map"]
    assert bits_equal(m, want), describe_diff(m, want, f"{name}: map")
    if masked:
        assert np.all(m == M.MAP_NODATA)      # the reference's line 465: with -mask nothing is ever written
    area = restate.inun_area(g["hand"], g["catch"], g["dxc"], g["dyc"], ids, depth)
    out = str(tmp_path / "depth.csv")
    restate.write_depths(out, ids, flow, depth, area, carea)
    assert open(out, "rb").read() == M.text_of(g["depth_csv_mask" if masked else "depth_csv"])


def test_goldens_cover_the_quirks():
    """The fixtures exercise what the semantics single out: hand cells at exactly 0 and at +-5e-7 (wet at every stage), nodata in all three
    rasters, ids the list does not have, a duplicated list id whose first block of rows is all zero, a zero-length reach (guarded columns stay
    0), unsorted stages with a repeat, and forecasts that end below, above, inside and exactly on the table, without rows, and at a depth <= 0."""
    for name in CASES:
        g = M.load_golden(name)
        hand, cat = g["hand"], g["catch"]
        assert np.sum(hand == 0.0) >= 8 and np.any(hand == np.float32(5e-7)) and np.any(hand == np.float32(-5e-7)), name
        assert np.any(hand < -1e30) and np.any(g["slp"] == -1.0) and np.any(cat == M.CATCH_NODATA), name
        rows = [ln.split(",") for ln in M.text_of(g["table_txt"]).decode().strip().split("\n")[1:]]
        listed = {int(r[0]) for r in rows}
        assert {64, 400} <= set(np.unique(cat).tolist()) and not ({64, 400} & listed), name
        seven = [r for r in rows if int(r[0]) == 7]
        assert len(seven) == 26 and all(int(r[2]) == 0 for r in seven[:13]) and any(int(r[2]) > 0 for r in seven[13:]), name
        five = [r for r in rows if int(r[0]) == 5]
        assert any(float(r[5]) > 0 for r in five) and all(float(r[9]) == 0 and float(r[13]) == 0 for r in five), name
        assert len(rows[0]) == 14 and (rows[0][12] == "0.050000") == (name == "rect_dxdy") or name != "rect_dxdy", name
        d = [ln.split(",") for ln in M.text_of(g["depth_csv"]).decode().strip().split("\n")[1:]]
        depth = {(int(r[0]), i): float(r[2]) for i, r in enumerate(d)}
        assert sum(v == -9999.0 for v in depth.values()) >= 5 and any(-9999.0 < v <= 0 for v in depth.values()) and any(v > 0 for v in depth.values()), name
        assert np.any(g["map"] > -1e30) and not np.any(g["map_mask"] > -1e30), name
