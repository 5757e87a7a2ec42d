"""read_polygon_layer through the library (taudem_amd.read_polygons), the attribute checks, the region table writer and the argument refusals of
siregiontool: host code, no GPU.  What write_polygon_layer writes is read back in both formats and agrees with the independent parser
tests/polygon_parse.py; shape types 15 and 25 come from bytes built here (tests/regiongrid_files.py)."""
import json
import os

import numpy as np
import pytest

import polygon_parse as P
import polygonize_model as PM
import regiongrid_files as F
import regiongrid_model as M
import taudem_amd as T
from taudem_amd import _lib, api, tools
from test_polygonize_model import HAND

GT = (440000.5, 30.0, 0.0, 4600000.25, 0.0, -30.0)
SQUARE = [(1.0, 1.0), (4.0, 1.0), (4.0, 3.0), (1.0, 3.0), (1.0, 1.0)]
TRIANGLE = [(0.5, 0.25), (2.5, 0.25), (1.5, 2.75), (0.5, 0.25)]


def _written(w, tmp_path, ext):
    m = PM.polygonize(w)
    path = str(tmp_path / ("layer" + ext))
    with T.Polygons(parts=[api.polygonize_edges_create(m.keys, m.next_keys, m.edge_ids)], nx=w.shape[1], ny=w.shape[0]) as pg:
        pg.write(path, GT)
    return path, m


def _rings(layer):
    return [[[tuple(p) for p in ring.tolist()] for ring in feat] for feat in layer.polygons]


@pytest.mark.parametrize("name", ["nested", "cut", "saddle", "all_nodata"])
def test_round_trip_through_the_library(name, tmp_path):
    w = HAND[name]
    want = np.where((w == PM.NODATA) | (w < 1), 0, w).astype(np.int16)
    shp, m = _written(w, tmp_path, ".shp")
    gj, _ = _written(w, tmp_path, ".geojson")
    a, b = T.read_polygons(shp), T.read_polygons(gj)
    assert _rings(a) == [rings for _, rings in P.shapefile_features(shp)]
    assert _rings(b) == [[ring for p in polys for ring in p] for _, polys in P.geojson(gj)[0]]
    ids = [i for i, _, _ in PM.features(m)]
    for layer in (a, b):
        assert len(layer) == len(ids) and [int(v) for v in layer.fields.get("gridcode", [])] == ids and set(layer.fields) == ({"gridcode", "cells"} if ids else set(layer.fields))
        keep = [k for k, i in enumerate(ids) if 1 <= i <= 32767]
        grid, _ = M.polygons(w.shape, GT, [layer.polygons[k] for k in keep], [ids[k] for k in keep])
        assert np.array_equal(grid, want), "the model burns the layer back into the grid it came from"


@pytest.mark.parametrize("shape_type", [5, 15, 25])
def test_shape_types_from_bytes(shape_type, tmp_path):
    feats = [[SQUARE, TRIANGLE], None, [TRIANGLE]]
    path = F.write_layer(str(tmp_path / "l.shp"), shape_type, feats, texts=["7", "8", "9"])
    layer = T.read_polygons(path)
    assert _rings(layer) == [[SQUARE, TRIANGLE], [], [TRIANGLE]] and layer.values("ID").tolist() == [7, 8, 9]
    assert layer.polygons[0][0].dtype == np.float64 and layer.polygons[0][0].shape == (5, 2)


def test_a_layer_of_another_type_or_extension_is_refused(tmp_path):
    path = str(tmp_path / "lines.shp")
    open(path, "wb").write(F.shp_bytes(3, []))
    with pytest.raises(T.TdxError, match="not a polygon layer"):
        T.read_polygons(path)
    with pytest.raises(T.TdxError, match="unsupported input") as e:
        T.read_polygons(str(tmp_path / "layer.gpkg"))
    assert e.value.code == -1
    with pytest.raises(T.TdxError, match="cannot open"):
        T.read_polygons(str(tmp_path / "missing.geojson"))


@pytest.mark.parametrize("text, why", [("", "is null"), ("1.5", "is not an integer"), ("0", "is outside 1 .. 32767"), ("32768", "is outside 1 .. 32767"),
                                       ("-3", "is outside"), ("abc", "is not an integer")])
def test_attribute_refusals(text, why, tmp_path):
    path = F.write_layer(str(tmp_path / "l.shp"), 5, [[SQUARE], [TRIANGLE]], texts=["4", text])
    layer = T.read_polygons(path)
    with pytest.raises(T.TdxError, match="feature 1: ID .*" + why) as e:
        layer.values("ID")
    assert e.value.code == -1
    gj = str(tmp_path / "l.geojson")
    value = "null" if text == "" else json.dumps(text) if text == "abc" else text
    open(gj, "w").write('{"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"ID": 4}, "geometry": {"type": "Polygon", "coordinates": '
                        '[[[1, 1], [4, 1], [4, 3], [1, 1]]]}}, {"type": "Feature", "properties": {"ID": %s}, "geometry": {"type": "MultiPolygon", "coordinates": '
                        '[[[[0, 0], [2, 0], [1, 2], [0, 0]]], [[[5, 5], [6, 5], [6, 6], [5, 5]]]]}}]}' % value)
    layer = T.read_polygons(gj)
    assert [len(f) for f in layer.polygons] == [1, 2]
    with pytest.raises(T.TdxError, match="feature 1: ID .*" + why):
        layer.values("ID")


def test_field_refusals_and_whole_reals(tmp_path):
    path = F.write_layer(str(tmp_path / "l.shp"), 5, [[SQUARE], [TRIANGLE]], texts=["4.000", "32767"], decimals=3)
    layer = T.read_polygons(path)
    assert layer.values("ID").tolist() == [4, 32767]
    with pytest.raises(T.TdxError, match="no field Region"):
        layer.values("Region")
    for fid in ("FID", "fid"):
        with pytest.raises(T.TdxError, match="FID is the record number"):
            layer.values(fid)


def test_table_writer(tmp_path):
    path = str(tmp_path / "att.csv")
    T.write_calpar(path, [3, 1, 32767])
    assert open(path, "rb").read() == M.table_text([3, 1, 32767]).encode()
    back = T.read_calpar(path)
    assert back["id"].tolist() == [3, 1, 32767] and back["tmin"].tolist() == [np.float32(2.708)] * 3 and back["rhos"].tolist() == [2000.0] * 3
    T.write_calpar(path, [2], tmin=0.1, tmax=1e-5, cmin=0, cmax=1, phimin=25.5, phimax=40, soildens=1800)
    assert open(path).read() == "SiID,tmin,tmax,cmin,cmax,phimin,phimax,SoilDens\n2,0.1,1e-05,0.0,1.0,25.5,40.0,1800.0\n"
    back = T.read_calpar(path)
    assert back["tmax"].tolist() == [np.float32(1e-5)] and back["phimin"].tolist() == [25.5]
    T.write_calpar(path, [])
    assert open(path).read() == "SiID,tmin,tmax,cmin,cmax,phimin,phimax,SoilDens\n" and T.read_calpar(path)["id"].size == 0
    with pytest.raises(T.TdxError) as e:
        T.write_calpar(str(tmp_path / "no" / "att.csv"), [1])
    assert e.value.code == 21


def test_tool_refusals_that_need_no_gpu(tmp_path, capfd):
    f = lambda s: str(tmp_path / s)  # noqa: E731
    before = sorted(os.listdir(tmp_path))
    assert tools.siregiontool(f("dem.tif"), f("parreg.tif"), f("att.csv"), parreg_in=f("r.tif"), shp=f("r.shp")) == -1
    assert "both given" in _lib.last_error()
    assert tools.siregiontool(f("dem.tif"), f("parreg.tif"), f("att.csv"), shp=f("r.gpkg")) == -1
    assert tools.siregiontool(f("dem.tif"), f("nowhere/parreg.tif"), f("att.csv")) == -1
    assert tools.siregiontool(f("dem.tif"), f("parreg.tif"), f("nowhere/att.csv")) == -1
    out = capfd.readouterr().out
    assert "version" not in out, "refused before anything is read: not even the banner"
    assert tools.siregiontool(f("missing.tif"), f("parreg.tif"), f("att.csv")) == 21      # the DEM is read first
    assert sorted(os.listdir(tmp_path)) == before
