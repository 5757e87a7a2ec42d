"""The device ring builder's schedule (tests/polygon_rings_device_model.py: min-jump rounds that also rank, rotation by the smallest vertex, owner
jumping, the three-pass sort key) held to the definition (tests/polygonize_model.py) without a GPU: on the grids of the GPU tests, on ring lengths on
both sides of every jump round, on the hole shapes and on 200 random grids.  The round count it needs never exceeds the bound the kernels use."""
import numpy as np
import pytest

import polygon_rings_device_model as D
import polygonize_model as M
from polygon_rings_cases import CASES, random_grid
from test_polygonize_model import HAND, RECORDED

ND = M.NODATA
GRIDS = dict(HAND, **{k: RECORDED[k] for k in ("plain:w_plain", "plain:w_outlets", "plain:w_sw", "holes:w_plain", "geographic:w_outlets")}, **CASES)


def held(w):
    m = M.polygonize(w)
    ny, nx = w.shape
    got, rounds = D.build(m.keys, m.next_keys, m.edge_ids, nx, ny)
    assert M.same(got, m)
    assert rounds.label <= rounds.bound and D.device_rounds(rounds.label, rounds.bound) <= rounds.bound
    assert rounds.owner <= rounds.owner_bound and D.device_rounds(rounds.owner, rounds.owner_bound) <= rounds.owner_bound
    return m, rounds


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_schedule_equals_the_definition(name):
    held(GRIDS[name])


def test_the_cases_are_what_they_claim():
    f = {name: M.features(M.polygonize(CASES[name])) for name in CASES}
    (a3, _, p3), (a7, _, p7) = f["serpentine_96x128"]
    assert (a3, len(p3), a7, len(p7)) == (3, 500, 7, 1) and all(len(p) == 1 and len(p[0]) == 5 for p in p3)
    assert 2 ** 13 < len(M.polygonize(CASES["serpentine_96x128"]).keys) - 2000 < 2 ** 14, "the long ring lies between two jump rounds"
    rings = lambda name: [(a, [len(p) for p in polys]) for a, _, polys in f[name]]  # noqa: E731
    assert rings("holes_stacked_3") == [(1, [4])] and rings("holes_stacked_5") == [(1, [6])]
    assert rings("holes_side_by_side") == [(1, [4])] and rings("hole_bottom_300x8") == [(1, [2])]
    assert rings("hole_island_hole") == [(1, [2, 2]), (2, [2, 2])]


@pytest.mark.parametrize("n", [31, 32, 33, 1023, 1024])
def test_ring_lengths_on_both_sides_of_a_round(n):
    m, rounds = held(np.full((1, n), 4, np.int32))
    E = 2 * n + 2
    assert len(m.keys) == E and rounds.bound == D.round_bound(E)
    assert rounds.label == int(np.ceil(np.log2(E))) + 1, "one ring of E edges: ceil(log2(E)) rounds to cover it and one that changes nothing"


def test_round_bound():
    assert [D.round_bound(n) for n in (1, 2, 3, 4, 5, 8, 9, 1 << 20, (1 << 20) + 1)] == [1, 2, 3, 3, 4, 4, 5, 21, 22]
    assert D.device_rounds(3, 5) == 4 and D.device_rounds(4, 5) == 4 and D.device_rounds(5, 5) == 5


@pytest.mark.parametrize("block", range(10))
def test_random_grids(block):
    for seed in range(20 * block, 20 * block + 20):
        held(random_grid(seed))


def test_malformed_edges_are_refused():
    w = HAND["cut"]
    ny, nx = w.shape
    m = M.polygonize(w)
    bad = m.next_keys.copy()
    bad[0] = bad[1]
    for keys, nxt, ids, why in ((m.keys[::-1].copy(), m.next_keys, m.edge_ids, "do not ascend"), (m.keys[5:], m.next_keys[5:], m.edge_ids[5:], "not among the edges"),
                                (m.keys, bad, m.edge_ids, "does not start|permutation"), (m.keys + 4 * nx * ny, m.next_keys, m.edge_ids, "outside the raster"),
                                (m.keys, m.next_keys, np.concatenate([m.edge_ids[:1] + 1, m.edge_ids[1:]]), "id changes")):
        with pytest.raises(D.Refused, match=why):
            D.build(keys, nxt, ids, nx, ny)
