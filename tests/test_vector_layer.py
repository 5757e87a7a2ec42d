"""The point-layer writer (taudem_amd/csrc/vector_layer.cpp through taudem_amd.write_points and the file path of moveoutletstostrm) read back by
tests/vector_parse.py, a reader written from the format descriptions that calls nothing of the product: record count and shape type, bounding box,
every coordinate bit for bit, field names, types and widths, the .shx offsets; GeoJSON with 17 significant digits.  A hand-made .dbf with N, F, C,
D and L columns comes out of moveoutletstostrm's outlet reader and layer writer with its bytes per column unchanged and Dist_moved appended (the
walk itself needs a GPU: tests/test_gpu_outlets_carryover.py); here the two halves are driven through tests/outlets/vector_main.cpp, the
stand-alone program that also runs under the sanitizers.  No GPU is needed."""
import os
import struct
import subprocess

import numpy as np
import pytest

import taudem_amd as T
import vector_parse as V
from taudem_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = np.array([1.5, -2.25, 1e-300, 123456789.12345679, np.nextafter(3.0, 4.0)], np.float64)
Y = np.array([10.0, 11.0, -12.5, 4.9e-324, 1.7976931348623157e308], np.float64)
FIELDS = {"id": np.array([1, -2, 3, 2147483647, -2147483648]), "Dist_moved": np.array([0, 1, -1, 50, 3], np.int32),
          "ad8": np.array([0.5, 12000.0, -0.0, 1e10, 3.0000001], np.float64), "name": ["a", "b c", "", "quote\"d", "x" * 90]}


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64).tolist()


def test_shapefile_reads_back(tmp_path):
    path = str(tmp_path / "pts.shp")
    T.write_points(path, X, Y, FIELDS)
    assert sorted(os.listdir(tmp_path)) == ["pts.dbf", "pts.shp", "pts.shx"]     # no .prj
    s, x, d = V.shp(path), V.shx(path[:-4] + ".shx"), V.dbf(path[:-4] + ".dbf")
    n = len(X)
    for h in (s, x):
        assert h["file_code"] == 9994 and h["unused"] == bytes(20) and h["version"] == 1000 and h["shape_type"] == 1
        assert bits(h["bbox"]) == bits([X.min(), Y.min(), X.max(), Y.max()]) and h["zm"] == (0.0, 0.0, 0.0, 0.0)
    assert [r[0] for r in s["records"]] == list(range(1, n + 1)) and all(r[1] == 10 and r[2] == 1 for r in s["records"])
    assert bits([r[3] for r in s["records"]]) == bits(X) and bits([r[4] for r in s["records"]]) == bits(Y)
    assert x["index"] == [(r[5], 10) for r in s["records"]] and x["index"][0] == (50, 10) and x["index"][1][0] == 64
    assert d["version"] == 3 and d["nrecords"] == n and d["terminator"] == 0x0D and d["eof"] == b"\x1a" and set(d["deleted"]) == {b" "}
    assert [(f[0], f[1], f[2], f[3]) for f in d["fields"]] == [("id", "N", 11, 0), ("Dist_moved", "N", 9, 0), ("ad8", "N", 24, 15), ("name", "C", 80, 0)]
    assert [int(r[0]) for r in d["rows"]] == FIELDS["id"].tolist() and [int(r[1]) for r in d["rows"]] == FIELDS["Dist_moved"].tolist()
    assert [float(r[2]) for r in d["rows"]] == [0.5, 12000.0, 0.0, 1e10, 3.0000001] and d["rows"][2][2].strip() == b"-0.000000000000000"
    assert d["rows"][1][3] == b"b c" + b" " * 77 and d["rows"][4][3] == b"x" * 80 and d["rows"][0][0] == b"          1"


def test_geojson_reads_back(tmp_path):
    path = str(tmp_path / "pts.geojson")
    T.write_points(path, X, Y, FIELDS)
    pts, text = V.geojson(path)
    assert bits([p[0] for p in pts]) == bits(X) and bits([p[1] for p in pts]) == bits(Y)
    assert [p[2]["id"] for p in pts] == FIELDS["id"].tolist() and [p[2]["name"] for p in pts] == ["a", "b c", None, "quote\"d", "x" * 90]
    assert bits([p[2]["ad8"] for p in pts]) == bits(FIELDS["ad8"]) and "123456789.12345679" in text and "3.0000000000000004" in text
    assert list(pts[0][2]) == ["id", "Dist_moved", "ad8", "name"]


@pytest.mark.parametrize("ext", [".shp", ".json", ".geojson"])
def test_empty_layer_and_read_outlets_round_trip(tmp_path, ext):
    empty = str(tmp_path / ("none" + ext))
    T.write_points(empty, [], [], {})
    if ext == ".shp":
        assert V.shp(empty)["records"] == [] and V.shx(empty[:-4] + ".shx")["index"] == [] and V.dbf(empty[:-4] + ".dbf")["nrecords"] == 0
    else:
        assert V.geojson(empty)[0] == []
    path = str(tmp_path / ("pts" + ext))
    ids = np.arange(1, len(X) + 1)
    T.write_points(path, X, Y, {"id": ids})
    lib = T.load()
    x, y, got = np.zeros(8), np.zeros(8), np.zeros(8, np.int32)
    import ctypes as C
    n = C.c_int64(0)
    assert lib.tdx_outlets_read(path.encode(), x.ctypes.data, y.ctypes.data, got.ctypes.data, 8, C.byref(n)) == 0 and n.value == len(X)
    assert bits(x[:5]) == bits(X) and bits(y[:5]) == bits(Y) and got[:5].tolist() == ids.tolist()


def test_other_extensions_are_refused(tmp_path):
    for name in ("pts.kml", "pts.sqlite", "pts", "pts.shp.txt"):
        with pytest.raises(_lib.TdxError) as e:
            T.write_points(str(tmp_path / name), X, Y, {})
        assert e.value.code == _lib.TDX_ERR_ARG and ".shp" in str(e.value) and ".geojson" in str(e.value)
    assert os.listdir(tmp_path) == []
    with pytest.raises(ValueError):
        T.write_points(str(tmp_path / "a.shp"), X, Y, {"id": [1, 2]})


# ---- carry-over, and the stand-alone program -----------------------------------------------------------------------------------------------
def hand_made_dbf(path, n):
    """N (9.0), F (13.4), C (7), D (8), L (1) columns with a non-zero reserved byte in a descriptor: what a byte-faithful copy must keep"""
    cols = [(b"GAGE_ID", b"N", 9, 0), (b"AREA_KM2", b"F", 13, 4), (b"NAME", b"C", 7, 0), (b"SINCE", b"D", 8, 0), (b"ACTIVE", b"L", 1, 0)]
    desc = b""
    for k, (name, t, wid, dec) in enumerate(cols):
        desc += name.ljust(11, b"\0") + t + b"\0\0\0\0" + bytes([wid, dec]) + bytes([0, 0, k + 1]) + bytes(11)
    rows = []
    for i in range(n):
        rows.append([b"%9d" % (100 + i), b"%13.4f" % (1.5 * i), (b"st %d" % i).ljust(7), b"1998%02d01" % (i % 12 + 1), b"TF?"[i % 3:i % 3 + 1]])
    rec = 1 + sum(c[2] for c in cols)
    b = struct.pack("<4BIHH", 3, 98, 7, 1, n, 32 + len(desc) + 1, rec) + bytes(20) + desc + b"\r" + b"".join(b" " + b"".join(r) for r in rows) + b"\x1a"
    open(path, "wb").write(b)
    return cols, rows


@pytest.fixture(scope="module")
def vector_main(tmp_path_factory):
    d = tmp_path_factory.mktemp("vector_main")
    exe = str(d / "vector_main")
    src = [os.path.join(ROOT, "tests", "outlets", "vector_main.cpp"), os.path.join(ROOT, "taudem_amd", "csrc", "vector_layer.cpp"),
           os.path.join(ROOT, "taudem_amd", "csrc", "outlets.cpp")]
    subprocess.run(["c++", "-O1", "-g", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "taudem_amd", "csrc")] + src + ["-o", exe], check=True)
    return exe


def test_stand_alone_program_writes_and_rereads_two_layers(vector_main, tmp_path):
    r = subprocess.run([vector_main, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.dbf", "a.shp", "a.shx", "b.geojson"]


@pytest.mark.parametrize("ext", [".shp", ".geojson"])
def test_dbf_columns_are_carried_over(vector_main, tmp_path, ext):
    n = 7
    src = str(tmp_path / "gages.shp")
    T.write_points(src, np.arange(n) * 2.5, np.arange(n) * -1.0, {})
    cols, rows = hand_made_dbf(src[:-4] + ".dbf", n)
    before = V.dbf(src[:-4] + ".dbf")
    out = str(tmp_path / ("moved" + ext))
    r = subprocess.run([vector_main, "carry", src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    if ext == ".shp":
        after = V.dbf(out[:-4] + ".dbf")
        assert [f[4] for f in after["fields"][:-1]] == [f[4] for f in before["fields"]]                      # the 32 descriptor bytes
        assert [row[:-1] for row in after["rows"]] == before["rows"] == rows                                  # the bytes of every column
        assert after["fields"][-1][:4] == ("Dist_moved", "N", 6, 0) and [row[-1] for row in after["rows"]] == [b"%6d" % (i - 1) for i in range(n)]
        assert bits([r[3] for r in V.shp(out)["records"]]) == bits(np.arange(n) * 2.5)
    else:
        pts, _ = V.geojson(out)
        assert [p[2]["GAGE_ID"] for p in pts] == [100 + i for i in range(n)] and [p[2]["AREA_KM2"] for p in pts] == [1.5 * i for i in range(n)]
        assert [p[2]["NAME"] for p in pts] == ["st %d" % i for i in range(n)] and pts[0][2]["SINCE"] == "19980101" and pts[2][2]["ACTIVE"] == "?"
        assert [p[2]["Dist_moved"] for p in pts] == [i - 1 for i in range(n)]
