"""PackedPolygons and Polygons.packed without a GPU: the constructor refuses offsets that do not cover their arrays, and the packed form of a polygon
set (built by the host ring builder from the model's edges) holds the same rings as Polygons.features(), which the model burns back into the grid."""
import numpy as np
import pytest

import polygonize_model as PM
import regiongrid_model as M
import taudem_amd as T
from taudem_amd import api
from test_polygonize_model import HAND

GT = (440000.5, 30.0, 0.0, 4600000.25, 0.0, -30.0)


def test_constructor_checks_the_offsets():
    p = T.PackedPolygons([0, 1, 1, 5, 6, 5], [0, 0, 1, 5, 5, 6], [0, 3, 6], [0, 1, 2])
    assert len(p) == 2 and p.x.dtype == np.float64 and p.ring_first.dtype == np.int64
    assert len(T.PackedPolygons([], [], [0], [0])) == 0
    for args in (([0, 1, 1], [0, 0], [0, 3], [0, 1]),            # unpaired coordinates
                 ([0, 1, 1], [0, 0, 1], [0, 2], [0, 1]),          # rings that do not cover the vertices
                 ([0, 1, 1], [0, 0, 1], [0, 3], [0, 2]),          # features that do not cover the rings
                 ([0, 1, 1], [0, 0, 1], [], [0, 1]),
                 ([0, 1, 1], [0, 0, 1], [0, 3], [])):
        with pytest.raises(ValueError, match="offsets"):
            T.PackedPolygons(*args)


@pytest.mark.parametrize("name", ["nested", "cut", "saddle", "ring_around_nodata", "all_nodata"])
def test_packed_holds_the_rings_of_the_features(name):
    w = HAND[name]
    m = PM.polygonize(w)
    with T.Polygons(parts=[api.polygonize_edges_create(m.keys, m.next_keys, m.edge_ids)], nx=w.shape[1], ny=w.shape[0]) as pg:
        pk, ids, feats = pg.packed(GT), pg.ids.copy(), pg.features()
    assert len(pk) == len(feats)
    rings = [[list(zip(pk.x[pk.ring_first[q]:pk.ring_first[q + 1]].tolist(), pk.y[pk.ring_first[q]:pk.ring_first[q + 1]].tolist()))
              for q in range(pk.feature_first[f], pk.feature_first[f + 1])] for f in range(len(pk))]
    assert rings == [[[(GT[0] + c * GT[1], GT[3] + r * GT[5]) for c, r in ring] for p in polys for ring in p] for _, _, polys in feats]
    x, y, ring_first, feature_first, vals = api._pack_polygons(pk, np.arange(1, len(pk) + 1))
    assert x is pk.x and ring_first is pk.ring_first and feature_first is pk.feature_first and vals.dtype == np.int32 and vals.tolist() == list(range(1, len(pk) + 1))
    keep = [k for k, i in enumerate(ids.tolist()) if 1 <= i <= 32767]
    grid, _ = M.polygons(w.shape, GT, [rings[k] for k in keep], [int(ids[k]) for k in keep])
    assert np.array_equal(grid, np.where((w == PM.NODATA) | (w < 1), 0, w))
