"""The polygon layer reader, the attribute checks and the region table writer in a stand-alone program (tests/regiongrid/reader_main.cpp) built with
-fsanitize=address,undefined -fno-sanitize-recover=all from vector_layer.cpp and region_table.cpp only, and run as a process of its own.  On good
files its text is the one made here from the same features; on files whose headers, record lengths, counts, part indices or .dbf record counts lie,
on GeoJSON cut short and on coordinates that are no numbers it prints "refused:" and ends with status 0 and an empty stderr: it never reads past a
buffer.  No GPU is needed and no sanitizer comes near code loaded into Python."""
import os
import struct
import subprocess

import pytest

import regiongrid_files as F
import regiongrid_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "taudem_amd", "csrc")
SQUARE = [(1.0, 1.0), (4.0, 1.0), (4.0, 3.0), (1.0, 3.0), (1.0, 1.0)]
TRIANGLE = [(440000.5, 4600000.25), (440060.125, 4600000.25), (440030.1, 4599940.7), (440000.5, 4600000.25)]
FEATURES = [[SQUARE, TRIANGLE], None, [TRIANGLE]]
GEOJSON = ('{"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"ID": 4}, "geometry": {"type": "Polygon", "coordinates": '
           '[[[1, 1], [4, 1], [4, 3], [1, 3], [1, 1]], [[2, 1.5], [3, 1.5], [2.5, 2.5], [2, 1.5]]]}}, {"type": "Feature", "properties": {"ID": 9}, '
           '"geometry": {"type": "MultiPolygon", "coordinates": [[[[0, 0], [2, 0], [1, 2], [0, 0]]], [[[5e0, 5], [6, 5], [6, 6.25], [5, 5]]]]}}]}')


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("polygon_reader") / "reader_main")
    subprocess.run(["c++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "regiongrid", "reader_main.cpp"), os.path.join(CSRC, "vector_layer.cpp"), os.path.join(CSRC, "region_table.cpp"),
                    "-o", out], check=True)
    return out


def _run(exe, *args):
    p = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (args, p.returncode, p.stderr)   # a sanitizer report goes to stderr and ends the process with a code
    return p.stdout


@pytest.mark.parametrize("shape_type", [5, 15, 25])
def test_good_shapefiles(exe, shape_type, tmp_path):
    path = F.write_layer(str(tmp_path / "l.shp"), shape_type, FEATURES, texts=["7", "8", "32767"])
    rings = [f or [] for f in FEATURES]
    assert _run(exe, "layer", path) == F.text_of(rings)
    assert _run(exe, "layer", path, "ID") == F.text_of(rings, [7, 8, 32767])
    assert _run(exe, "layer", path, "FID").startswith("refused: the field FID")
    assert _run(exe, "layer", path, "Region").startswith("refused: the polygon layer has no field Region")


def test_good_geojson_and_table(exe, tmp_path):
    path = str(tmp_path / "l.geojson")
    open(path, "w").write(GEOJSON)
    rings = [[SQUARE, [(2.0, 1.5), (3.0, 1.5), (2.5, 2.5), (2.0, 1.5)]], [[(0.0, 0.0), (2.0, 0.0), (1.0, 2.0), (0.0, 0.0)], [(5.0, 5.0), (6.0, 5.0), (6.0, 6.25), (5.0, 5.0)]]]
    assert _run(exe, "layer", path, "ID") == F.text_of(rings, [4, 9])
    assert _run(exe, "table", tmp_path / "att.csv", 1, 5, 32767) == M.table_text([1, 5, 32767])
    assert _run(exe, "table", tmp_path / "nowhere" / "att.csv", 1).startswith("refused: cannot write")


def _malformed_shapefiles():
    good = F.shp_bytes(5, [F.record(5, f) for f in FEATURES])
    rec = F.record(5, [SQUARE, TRIANGLE])
    poke = lambda b, at, fmt, v: b[:at] + struct.pack(fmt, v) + b[at + struct.calcsize(fmt):]  # noqa: E731
    return {
        "truncated_header": good[:60],
        "truncated_in_a_record": good[:100 + 8 + 60],
        "truncated_in_a_record_header": good[:100 + 8 + len(rec) + 5],
        "record_length_beyond_the_file": poke(good, 104, ">i", 1 << 20),
        "record_length_negative": poke(good, 104, ">i", -4),
        "part_index_beyond_the_points": F.shp_bytes(5, [poke(rec, 48, "<i", 77)]),
        "part_indices_descending": F.shp_bytes(5, [poke(poke(rec, 44, "<i", 6), 48, "<i", 2)]),
        "point_count_overflows": F.shp_bytes(5, [poke(rec, 40, "<i", -1)]),
        "point_count_beyond_the_record": F.shp_bytes(5, [poke(rec, 40, "<i", len(SQUARE) + len(TRIANGLE) + 1)]),
        "part_count_overflows": F.shp_bytes(5, [poke(rec, 36, "<i", 0x7fffffff)]),
        "short_record": F.shp_bytes(5, [rec[:40]]),
        "wrong_magic": poke(good, 0, ">i", 9995),
    }


@pytest.mark.parametrize("name", sorted(_malformed_shapefiles()))
def test_malformed_shapefiles_are_refused(exe, name, tmp_path):
    path = str(tmp_path / "l.shp")
    open(path, "wb").write(_malformed_shapefiles()[name])
    open(path[:-4] + ".dbf", "wb").write(F.dbf_bytes("ID", ["1", "2", "3"]))
    assert _run(exe, "layer", path, "ID").startswith("refused: "), name


def test_malformed_tables_are_refused(exe, tmp_path):
    path = F.write_layer(str(tmp_path / "l.shp"), 5, FEATURES, texts=["1", "2"])                       # fewer records than shapes
    assert _run(exe, "layer", path, "ID").startswith("refused: the .dbf next to")
    F.write_layer(path, 5, FEATURES, texts=["1", "2"], nrecords=3)                                     # a count its bytes do not hold
    assert _run(exe, "layer", path, "ID").startswith("refused: the .dbf next to")
    open(path[:-4] + ".dbf", "wb").write(F.dbf_bytes("ID", ["1", "2", "3"])[:20])
    assert _run(exe, "layer", path, "ID").startswith("refused: not a .dbf file")
    for text, why in (("", "is null"), ("1.5", "is not an integer"), ("0", "is outside"), ("32768", "is outside"), ("**********", "is null")):
        F.write_layer(path, 5, FEATURES, texts=["1", "2", text])
        assert "feature 2: ID" in _run(exe, "layer", path, "ID") and why in _run(exe, "layer", path, "ID")


@pytest.mark.parametrize("name, text", [
    ("cut_mid_array", GEOJSON[:GEOJSON.index("[4, 3]") + 3]),
    ("cut_mid_number", GEOJSON[:GEOJSON.index("6.25") + 2]),
    ("cut_mid_string", GEOJSON[:GEOJSON.index("MultiPolygon") + 5]),
    ("coordinates_are_strings", GEOJSON.replace("[4, 1]", '["4", "1"]')),
    ("coordinates_are_words", GEOJSON.replace("[4, 1]", "[four, 1]")),
    ("coordinates_are_half_numbers", GEOJSON.replace("[4, 1]", "[4e, 1-]")),
    ("a_position_of_one_number", GEOJSON.replace("[4, 1]", "[4]")),
    ("a_ring_that_is_a_number", GEOJSON.replace("[[[0, 0], [2, 0], [1, 2], [0, 0]]]", "[7]")),
    ("a_polygon_that_is_a_number", GEOJSON.replace("[[[[0, 0], [2, 0], [1, 2], [0, 0]]],", "[3,")),
    ("trailing_garbage", GEOJSON + "]"),
    ("empty", ""),
])
def test_malformed_geojson_is_refused(exe, name, text, tmp_path):
    path = str(tmp_path / "l.geojson")
    open(path, "w").write(text)
    assert _run(exe, "layer", path, "ID").startswith("refused: "), name
