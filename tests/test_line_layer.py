"""Line layers (taudem_amd/csrc/vector_layer.cpp: write_line_layer, read_line_layer, through tdx_lines_write / tdx_lines_read): the round trip write -> read for
.shp and .geojson with a line of a single vertex; the .shp / .shx / .dbf headers and record lengths read back with the tests' own parsers; shape types 13
and 23 (and several parts, of which the first is taken) from bytes the test builds; any other extension refused.  No GPU is needed."""
import json
import os

import numpy as np
import pytest

import line_parse as LP
import taudem_amd as T
import vector_parse as V
from taudem_amd import _lib

LINES = [np.array([[1.5, 10.0], [2.5, 9.0], [4.0, 8.5]]), np.array([[7.25, -3.0]]), np.array([[0.1, 0.3], [0.2, 0.4]]), np.array([[1e6 + 1 / 3, -2e6 - 1 / 7], [5.0, 5.0]])]
FIELDS = {"LINKNO": np.array([1, -2, 3, 400000]), "Length": np.array([12.5, 0.0, -3.5, 1234567.891]), "Slope": np.array([0.1, 1 / 3, 0.0, 2e-9]), "name": ["a", "", "c c", "d"]}
WIDTHS = {"LINKNO": (6, 0), "Length": (16, 1), "Slope": (16, 12)}


@pytest.mark.parametrize("ext", [".shp", ".geojson", ".json"])
def test_round_trip(tmp_path, ext):
    path = str(tmp_path / ("l" + ext))
    T.write_lines(path, LINES, FIELDS, WIDTHS)
    lines, fields = T.read_lines(path)
    assert len(lines) == 4 and all(a.tobytes() == b.tobytes() for a, b in zip(lines, LINES))   # a line of one vertex comes back as one
    assert list(fields) == list(FIELDS) and fields["LINKNO"].tolist() == FIELDS["LINKNO"].tolist() and fields["name"] == FIELDS["name"]
    if ext == ".shp":   # the .dbf holds what its decimals keep
        assert fields["Length"].tolist() == [12.5, 0.0, -3.5, 1234567.9] and fields["Slope"].tolist() == [0.1, 0.333333333333, 0.0, 2e-9]
        assert sorted(os.listdir(tmp_path)) == ["l.dbf", "l.shp", "l.shx"]
    else:
        assert fields["Length"].tobytes() == FIELDS["Length"].tobytes() and fields["Slope"].tobytes() == FIELDS["Slope"].tobytes()   # 17 significant digits
        doc = json.loads(open(path).read())
        assert [f["geometry"]["type"] for f in doc["features"]] == ["LineString"] * 4 and doc["features"][1]["geometry"]["coordinates"] == [[7.25, -3.0]]
        assert doc["features"][1]["properties"]["name"] is None and doc["features"][3]["properties"]["LINKNO"] == 400000


def test_shapefile_bytes(tmp_path):
    path = str(tmp_path / "l.shp")
    T.write_lines(path, LINES, FIELDS, WIDTHS)
    s, x, d = LP.polylines(path), V.shx(path[:-4] + ".shx"), V.dbf(path[:-4] + ".dbf")
    allpts = np.concatenate(LINES)
    box = (allpts[:, 0].min(), allpts[:, 1].min(), allpts[:, 0].max(), allpts[:, 1].max())
    for h in (s, x):
        assert h["file_code"] == 9994 and h["version"] == 1000 and h["shape_type"] == 3 and h["bbox"] == box and h["zm"] == (0, 0, 0, 0) and h["unused"] == b"\0" * 20
    assert [r[0] for r in s["records"]] == [1, 2, 3, 4]
    for r, v in zip(s["records"], LINES):
        assert r[1] == 24 + 8 * len(v) and r[2] == 3 and r[4] == [0] and r[5].tobytes() == v.tobytes()   # one part that starts at vertex 0
        assert r[3] == (v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max())
    assert x["index"] == [(r[6], r[1]) for r in s["records"]]   # offsets and content lengths in 16-bit words
    assert [(f[0], f[1], f[2], f[3]) for f in d["fields"]] == [("LINKNO", "N", 6, 0), ("Length", "N", 16, 1), ("Slope", "N", 16, 12), ("name", "C", 80, 0)]
    assert d["nrecords"] == 4 and d["header_bytes"] == 32 + 4 * 32 + 1 and d["record_bytes"] == 1 + 6 + 16 + 16 + 80 and d["eof"] == b"\x1a" and d["terminator"] == 0x0D
    assert d["rows"][3][0] == b"400000" and d["rows"][0][1] == b"12.5".rjust(16) and d["rows"][1][2] == b"0.333333333333".rjust(16) and d["rows"][1][3] == b" " * 80
    # the same layer, the same bytes
    again = str(tmp_path / "m.shp")
    T.write_lines(again, LINES, FIELDS, WIDTHS)
    for e in (".shp", ".shx", ".dbf"):
        assert open(path[:-4] + e, "rb").read() == open(again[:-4] + e, "rb").read()


@pytest.mark.parametrize("shape_type", [3, 13, 23])
def test_reads_z_and_m_types_and_the_first_part(tmp_path, shape_type):
    lines = [[[1, 2], [3, 4], [5, 6], [7, 8], [9, 10]], [[20, 21]], [[30, 31], [32, 33]]]
    path = str(tmp_path / "z.shp")
    open(path, "wb").write(LP.build_shp(shape_type, lines, parts_of={0: [0, 3]}))   # the first line has two parts: vertices 0..2 and 3..4
    open(path[:-4] + ".dbf", "wb").write(LP.build_dbf(3))
    got, fields = T.read_lines(path)
    assert [g.tolist() for g in got] == [[[1, 2], [3, 4], [5, 6]], [[20, 21]], [[30, 31], [32, 33]]] and fields["ID"].tolist() == [1, 2, 3]
    open(path[:-4] + ".dbf", "wb").write(LP.build_dbf(2))   # a table of another length is not taken
    with pytest.raises(_lib.TdxError) as e:
        T.read_lines(path)
    assert e.value.code == _lib.TDX_ERR_FILE


def test_refusals(tmp_path):
    for ext in (".kml", ".gpkg", ""):
        with pytest.raises(_lib.TdxError) as e:
            T.write_lines(str(tmp_path / ("l" + ext)), LINES, FIELDS)
        assert e.value.code == _lib.TDX_ERR_ARG and ".shp" in str(e.value) and ".geojson" in str(e.value)
        with pytest.raises(_lib.TdxError) as e:
            T.read_lines(str(tmp_path / ("l" + ext)))
        assert e.value.code == _lib.TDX_ERR_ARG
    assert not os.listdir(tmp_path)
    with pytest.raises(_lib.TdxError) as e:
        T.read_lines(str(tmp_path / "missing.shp"))
    assert e.value.code == _lib.TDX_ERR_FILE
    pts = str(tmp_path / "points.shp")   # a point layer is no line layer; a record that claims more vertices than it holds is refused, not read
    T.write_points(pts, [1.0, 2.0], [3.0, 4.0], {"id": np.array([1, 2])})
    with pytest.raises(_lib.TdxError):
        T.read_lines(pts)
    b = bytearray(LP.build_shp(3, [[[1, 2], [3, 4]]]))
    b[100 + 8 + 40:100 + 8 + 44] = (1000).to_bytes(4, "little")
    open(str(tmp_path / "bad.shp"), "wb").write(bytes(b))
    with pytest.raises(_lib.TdxError) as e:
        T.read_lines(str(tmp_path / "bad.shp"))
    assert e.value.code == _lib.TDX_ERR_FILE and "impossible" in str(e.value)
    with pytest.raises(ValueError):
        T.write_lines(str(tmp_path / "l.shp"), LINES, {"a": [1, 2]})
    T.write_lines(str(tmp_path / "empty.geojson"), [], {})
    assert T.read_lines(str(tmp_path / "empty.geojson")) == ([], {})
