"""The polygon layer writer (tdx_polygons_write, Polygons.write) read back through tests/polygon_parse.py, on a machine without a GPU: the polygons come
from the model's edges through the host ring builder.
  shapefile  header (file code, version, shape type 5, lengths), the bbox of the file and of every record, part and point counts, content lengths,
             .shx offsets, .dbf descriptors (gridcode N 10, cells N 12) and values; rings as parts in the layer's order, outer rings clockwise;
  GeoJSON    Polygon for one polygon, MultiPolygon otherwise, holes grouped with their outer ring, every ring reversed (RFC 7946: exterior rings
             counter-clockwise, holes clockwise) from and to the same start vertex, 17 significant digits;
  both       the same bytes twice, world coordinates x = gt[0] + c * gt[1], y = gt[3] + r * gt[5], the empty layer, a refused extension."""
import os
import struct

import numpy as np
import pytest

import polygon_parse as P
import polygonize_model as M
import taudem_amd as T
import vector_parse as V
from taudem_amd import _lib, api
from test_polygonize_model import HAND

GT = (1000.25, 30.0, 0.0, 5000.5, 0.0, -10.0)
CASES = ("nested", "cut", "saddle", "one_cell", "negative_and_zero")


def polygons_of(w):
    m = M.polygonize(w)
    return m, T.Polygons(parts=[api.polygonize_edges_create(m.keys, m.next_keys, m.edge_ids)], nx=w.shape[1], ny=w.shape[0])


def world(ring):
    return [(GT[0] + c * GT[1], GT[3] + r * GT[5]) for c, r in ring]


@pytest.mark.parametrize("name", CASES)
def test_shapefile(name, tmp_path):
    w = HAND[name]
    m, pg = polygons_of(w)
    path = str(tmp_path / "poly.shp")
    with pg:
        pg.write(path, GT)
        first = {e: open(path[:-4] + e, "rb").read() for e in (".shp", ".shx", ".dbf")}
        pg.write(path, GT)
    assert sorted(os.listdir(tmp_path)) == ["poly.dbf", "poly.shp", "poly.shx"]   # no .prj
    assert first == {e: open(path[:-4] + e, "rb").read() for e in (".shp", ".shx", ".dbf")}, "the same bytes twice"
    feats = M.features(m)
    s, x, d = P.shp(path), V.shx(path[:-4] + ".shx"), V.dbf(path[:-4] + ".dbf")
    assert s["file_code"] == 9994 and s["version"] == 1000 and s["shape_type"] == 5 and s["unused"] == bytes(20) and s["zm"] == (0.0,) * 4
    assert x["shape_type"] == 5 and x["bbox"] == s["bbox"] and x["file_words"] == 50 + 4 * len(feats)
    allpts = [v for _, _, polys in feats for p in polys for ring in p for v in world(ring)]
    assert s["bbox"] == (min(v[0] for v in allpts), min(v[1] for v in allpts), max(v[0] for v in allpts), max(v[1] for v in allpts))
    assert len(s["records"]) == len(feats) == len(x["index"])
    for k, (rec, (a, cells, polys)) in enumerate(zip(s["records"], feats)):
        want = [world(ring) for p in polys for ring in p]   # every ring a part: the outer ring of a polygon, then its holes
        pts = [v for ring in want for v in ring]
        assert rec[0] == k + 1 and rec[2] == 5 and rec[1] == 22 + 2 * len(want) + 8 * len(pts)
        assert x["index"][k] == (rec[6], rec[1])
        assert rec[3] == (min(v[0] for v in pts), min(v[1] for v in pts), max(v[0] for v in pts), max(v[1] for v in pts))
        assert P.rings(rec) == want
        outer_at = set(np.cumsum([0] + [len(p) for p in polys])[:-1].tolist())
        for q, ring in enumerate(P.rings(rec)):
            assert ring[0] == ring[-1] and (P.area2(ring) < 0) == (q in outer_at), "outer rings clockwise, holes counter-clockwise"
    wid = max([10] + [len(str(a)) for a, _, _ in feats])   # width 10; the writer widens an Integer column to its longest value: -2147483648 has 11 characters
    assert [(f[0], f[1], f[2], f[3]) for f in d["fields"]] == [("gridcode", "N", wid, 0), ("cells", "N", 12, 0)]
    assert d["nrecords"] == len(feats) and d["terminator"] == 0x0D and d["eof"] == b"\x1a"
    assert [[int(v) for v in row] for row in d["rows"]] == [[a, cells] for a, cells, _ in feats]
    assert all(len(row[0]) == wid and len(row[1]) == 12 for row in d["rows"])
    assert [f["gridcode"] for f, _ in P.shapefile_features(path)] == [str(a) for a, _, _ in feats]


@pytest.mark.parametrize("ext", [".geojson", ".json"])
@pytest.mark.parametrize("name", CASES)
def test_geojson(name, ext, tmp_path):
    w = HAND[name]
    m, pg = polygons_of(w)
    path = str(tmp_path / ("poly" + ext))
    with pg:
        pg.write(path, GT)
        first = open(path, "rb").read()
        pg.write(path, GT)
    assert os.listdir(tmp_path) == ["poly" + ext] and first == open(path, "rb").read()
    feats = M.features(m)
    got, text = P.geojson(path)
    assert len(got) == len(feats)
    for (props, polys), (a, cells, want) in zip(got, feats):
        assert props == {"gridcode": a, "cells": cells}
        assert polys == [[world(ring)[::-1] for ring in p] for p in want], "holes with their outer ring, every ring reversed"
        for p, wp in zip(polys, want):
            for q, (ring, wr) in enumerate(zip(p, wp)):
                assert ring[0] == ring[-1] == world(wr)[0]
                assert (P.area2(ring) > 0) == (q == 0), "RFC 7946: exterior counter-clockwise, holes clockwise"
    for v in (GT[0] + GT[1], GT[3] + GT[5]):
        assert ("%.17g" % v) in text


def test_world_coordinates_are_the_formula_in_double(tmp_path):
    gt = (0.1, 0.3, 0.0, 7.7, 0.0, -0.7)
    w = np.full((3, 5), 4, np.int32)
    m, pg = polygons_of(w)
    with pg:
        pg.write(str(tmp_path / "a.shp"), gt)
    (rec,) = P.shp(str(tmp_path / "a.shp"))["records"]
    want = [(gt[0] + c * gt[1], gt[3] + r * gt[5]) for c, r in [(0, 0), (5, 0), (5, 3), (0, 3), (0, 0)]]
    assert [struct.pack("<2d", *v) for v in rec[5]] == [struct.pack("<2d", *v) for v in want]


@pytest.mark.parametrize("ext", [".shp", ".geojson"])
def test_empty_layer(ext, tmp_path):
    _, pg = polygons_of(HAND["all_nodata"])
    path = str(tmp_path / ("none" + ext))
    with pg:
        pg.write(path, GT)
    if ext == ".shp":
        s, x, d = P.shp(path), V.shx(path[:-4] + ".shx"), V.dbf(path[:-4] + ".dbf")
        assert s["records"] == [] and s["file_words"] == 50 and s["shape_type"] == 5 and s["bbox"] == (0.0,) * 4 and x["index"] == []
        assert d["nrecords"] == 0 and [f[0] for f in d["fields"]] == ["gridcode", "cells"]
    else:
        assert P.geojson(path)[0] == []


def test_refused_extension(tmp_path):
    _, pg = polygons_of(HAND["one_cell"])
    with pg:
        for name in ("poly.gpkg", "poly", "poly.shp.txt"):
            with pytest.raises(T.TdxError, match="unsupported output") as e:
                pg.write(str(tmp_path / name), GT)
            assert e.value.code == _lib.TDX_ERR_ARG
        with pytest.raises(ValueError):
            pg.write(str(tmp_path / "poly.shp"), GT[:4])
    assert os.listdir(tmp_path) == []
