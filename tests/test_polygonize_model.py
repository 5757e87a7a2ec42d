"""The model of the watershed polygons (tests/polygonize_model.py) against its own checkers - the rings fill back to exactly w == id, cells counts the
cells, every id has as many polygons as 4-connected pieces, the orders of the layer hold - on every recorded w grid of tests/golden/streamnet_*.npz and
on the hand cases, and against three tiny cases whose ring lists are written out here by hand.  No GPU and no library."""
import glob
import os

import numpy as np
import pytest

import polygonize_model as M
from conftest import GOLDEN_DIR


def recorded_w():
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN_DIR, "streamnet_*.npz"))):
        g = np.load(path, allow_pickle=False)
        for k in g.files:
            if (k.startswith("w_") or "_w_" in k) and g[k].ndim == 2:
                out[os.path.basename(path)[10:-4] + ":" + k] = g[k].astype(np.int32)
    return out


RECORDED = recorded_w()
HAND = M.hand_cases()


def test_there_are_recorded_grids():
    assert len(RECORDED) == 45 and any(k.endswith(":w_plain") for k in RECORDED)


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_model_on_recorded_grid(name):
    w = RECORDED[name]
    M.check(w, M.polygonize(w))


@pytest.mark.parametrize("name", sorted(HAND))
def test_model_on_hand_case(name):
    w = HAND[name]
    m = M.polygonize(w)
    M.check(w, m)
    assert np.all(np.diff(m.keys) > 0) and set(m.next_keys.tolist()) == set(m.keys.tolist())


def test_multi_part_features_exist():
    """A D8 watershed is 8-connected: on a recorded grid some id has more than one polygon."""
    m = M.polygonize(next(RECORDED[k] for k in sorted(RECORDED) if k.endswith(":w_plain")))
    assert len(m.ring_first) - 1 > len(m.ids)


def test_one_cell_by_hand():
    assert M.features(M.polygonize(HAND["one_cell"])) == [(7, 1, [[[(0, 0), (1, 0), (1, 1), (0, 1), (0, 0)]]])]


def test_saddle_by_hand():
    """[[1, 2], [2, 1]]: four rings of four vertices, two features of two polygons: turning right keeps the pieces that touch at (1, 1) apart."""
    sq = lambda c, r: [[(c, r), (c + 1, r), (c + 1, r + 1), (c, r + 1), (c, r)]]  # noqa: E731
    assert M.features(M.polygonize(HAND["saddle"])) == [(1, 2, [sq(0, 0), sq(1, 1)]), (2, 2, [sq(1, 0), sq(0, 1)])]


def test_ring_around_nodata_by_hand():
    """One outer ring, clockwise in map view, and one hole, counter-clockwise, that starts at the hole's smallest vertex."""
    outer = [(0, 0), (3, 0), (3, 3), (0, 3), (0, 0)]
    hole = [(1, 1), (1, 2), (2, 2), (2, 1), (1, 1)]
    assert M.features(M.polygonize(HAND["ring_around_nodata"])) == [(1, 8, [[outer, hole]])]


def test_empty_layer():
    m = M.polygonize(HAND["all_nodata"])
    assert m.ids.size == 0 and m.keys.size == 0 and m.poly_first.tolist() == [0] and m.ring_first.tolist() == [0] and m.vert_first.tolist() == [0]


def test_nested_island_is_its_own_polygon():
    """id 1 with a hole of id 2 that holds an island of id 1: the island is a second polygon of feature 1, not a ring of the first."""
    feats = M.features(M.polygonize(HAND["nested"]))
    assert [f[0] for f in feats] == [1, 2]
    assert [len(p) for p in feats[0][2]] == [2, 1] and [len(p) for p in feats[1][2]] == [2]
