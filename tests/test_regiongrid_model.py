"""tests/regiongrid_model.py on hand cases whose answers are written out: the contract of include/taudem_amd_regions.h, rule by rule.  The GPU tests
hold the product to the model; this file holds the model to the definition."""
import numpy as np
import pytest

import regiongrid_model as M

GT = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0)   # world coordinates are pixel coordinates


def _rows(*rows):
    return np.array([[int(ch) for ch in r] for r in rows], np.int16)


def _box(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


SQUARE = _rows("000000", "011100", "011100", "000000", "000000")
DIAMOND = _rows("00000000", "00011000", "00111100", "01111110", "00111100", "00011000", "00000000", "00000000")
HOLE_ISLAND = _rows("11111111", "10000001", "10000001", "10011001", "10011001", "10000001", "10000001", "11111111")

# name -> (shape, features, values, expected grid)
HAND_CASES = {
    # corners on cell corners: rows 1, 2 (centres 1.5, 2.5 in [1, 3)), columns 1 .. 3 (centres right of 1, not right of 4)
    "square": ((5, 6), [[_box(1, 1, 4, 3)]], [1], SQUARE),
    # all four vertices on cell centres: the top vertex (a local extremum on row 0's scanline) counts twice, the bottom one (row 6) not at all, the
    # side vertices once; the edge through the centre of cell (2, 1) leaves that cell outside (xs < xc is strict), the one through (4, 1) inside
    "diamond": ((8, 8), [[[(3.5, 0.5), (6.5, 3.5), (3.5, 6.5), (0.5, 3.5), (3.5, 0.5)]]], [1], DIAMOND),
    # the top edge lies on row 1's scanline and the bottom edge on row 3's: horizontal edges never cross; the sides span [1.5, 3.5): rows 1, 2
    "horizontal": ((5, 6), [[_box(1, 1.5, 5, 3.5)]], [1], _rows("000000", "011110", "011110", "000000", "000000")),
    "hole_island": ((8, 8), [[_box(0, 0, 8, 8), _box(1, 1, 7, 7), _box(3, 3, 5, 5)]], [1], HOLE_ISLAND),
    # two rings of ONE feature: where they overlap, even-odd cancels
    "self_overlap": ((6, 6), [[_box(0, 0, 4, 4), _box(2, 2, 6, 6)]], [1], _rows("111100", "111100", "110011", "110011", "001111", "001111")),
    # the same rings as two features: the later one wins
    "two_features": ((6, 6), [[_box(0, 0, 4, 4)], [_box(2, 2, 6, 6)]], [3, 7], _rows("333300", "333300", "337777", "337777", "007777", "007777")),
    "later_loses_nothing": ((6, 6), [[_box(2, 2, 6, 6)], [_box(0, 0, 4, 4)]], [7, 3], _rows("333300", "333300", "333377", "333377", "007777", "007777")),
    "unclosed": ((5, 6), [[_box(1, 1, 4, 3)[:-1]]], [1], SQUARE),
    "two_vertices": ((5, 6), [[[(1, 1), (4, 3)]], [[(1, 1), (4, 3), (1, 1)]]], [1, 2], np.zeros((5, 6), np.int16)),
}


@pytest.mark.parametrize("name", list(HAND_CASES))
def test_hand_case(name):
    shape, features, values, want = HAND_CASES[name]
    grid, ids = M.polygons(shape, GT, features, values)
    assert grid.dtype == np.int16 and np.array_equal(grid, want)
    assert np.array_equal(ids, sorted(set(want[want != 0].tolist())))


def test_flipped_rows_and_scaled_cells():
    """gt[5] < 0 (a north-up raster) and cells of 10 x 25: the square at the same cells."""
    gt = (100.0, 10.0, 0.0, 500.0, 0.0, -25.0)
    ring = [(100 + 10 * x, 500 - 25 * y) for x, y in _box(1, 1, 4, 3)]
    grid, _ = M.polygons((5, 6), gt, [[ring]], [9])
    assert np.array_equal(grid, SQUARE * 9)


def test_strip_rows_are_the_rasters_rows():
    shape, features, values, want = HAND_CASES["diamond"]
    grid, ids = M.polygons((3, 8), GT, features, values, row0=2)
    assert np.array_equal(grid, want[2:5]) and ids.tolist() == [1]


def test_values_outside_int16_are_refused():
    for v in (0, -1, 32768):
        with pytest.raises(ValueError, match="feature 1"):
            M.polygons((5, 6), GT, [[_box(1, 1, 4, 3)]] * 2, [1, v])


def test_resample_by_hand():
    src = np.array([[1, 2], [3, -9]], np.int32)   # cells of 2 x 2 from (1, 1): covers x, y in [1, 5)
    grid, ids, bad = M.resample((6, 6), GT, src, (1.0, 2.0, 0.0, 1.0, 0.0, 2.0), -9)
    assert np.array_equal(grid, _rows("000000", "011220", "011220", "033000", "033000", "000000")) and ids.tolist() == [1, 2, 3] and bad == 0
    src[0, 0] = 40000
    src[1, 0] = 0
    grid, ids, bad = M.resample((6, 6), GT, src, (1.0, 2.0, 0.0, 1.0, 0.0, 2.0), -9)
    assert bad == 8 and ids.tolist() == [2]


def test_constant_and_table():
    grid, ids = M.constant((3, 4))
    assert np.array_equal(grid, np.ones((3, 4), np.int16)) and ids.tolist() == [1]
    assert M.table_text([1, 5]) == ("SiID,tmin,tmax,cmin,cmax,phimin,phimax,SoilDens\n1,2.708,2.708,0.0,0.25,30.0,45.0,2000.0\n"
                                    "5,2.708,2.708,0.0,0.25,30.0,45.0,2000.0\n")
