"""A reader of polygon layers for the tests, next to vector_parse.py (whose header, .shx and .dbf readers it uses): written from the ESRI Shapefile
Technical Description (July 1998, shape type 5) and RFC 7946, and calling nothing of the product.

    shp(path)       -> the header fields of vector_parse.shp and records [(number, words, type, bbox, parts [first point of every ring], points [(x, y)],
                       offset in words)]
    rings(record)   -> [[(x, y), ...]] the record's parts as point lists
    geojson(path)   -> [(properties, [polygon, ...])] with polygon = [ring, ...] and ring = [(x, y), ...], and the text
    shapefile_features(path) -> [({field: stripped text}, [ring, ...])] of a .shp and its .dbf
"""
import json
import struct

import vector_parse as V


def shp(path):
    b = open(path, "rb").read()
    h = V._header(b)
    assert h["file_words"] * 2 == len(b), "the header's length is the file's"
    recs, pos = [], 100
    while pos < len(b):
        number, words = struct.unpack(">ii", b[pos:pos + 8])
        body = b[pos + 8:pos + 8 + 2 * words]
        assert len(body) == 2 * words
        t, = struct.unpack("<i", body[:4])
        box = struct.unpack("<4d", body[4:36])
        nparts, npoints = struct.unpack("<ii", body[36:44])
        assert 2 * words == 44 + 4 * nparts + 16 * npoints, "the content length is that of the counts"
        parts = list(struct.unpack(f"<{nparts}i", body[44:44 + 4 * nparts]))
        flat = struct.unpack(f"<{2 * npoints}d", body[44 + 4 * nparts:])
        recs.append((number, words, t, box, parts, list(zip(flat[0::2], flat[1::2])), pos // 2))
        pos += 8 + 2 * words
    assert pos == len(b)
    h["records"] = recs
    return h


def rings(rec):
    parts, pts = rec[4], rec[5]
    assert parts == sorted(parts) and (not parts or parts[0] == 0)
    return [pts[a:b] for a, b in zip(parts, parts[1:] + [len(pts)])]


def geojson(path):
    text = open(path).read()
    doc = json.loads(text)
    assert doc["type"] == "FeatureCollection"
    out = []
    for f in doc["features"]:
        assert f["type"] == "Feature"
        g = f["geometry"]
        assert g["type"] in ("Polygon", "MultiPolygon")
        polys = [g["coordinates"]] if g["type"] == "Polygon" else g["coordinates"]
        assert g["type"] == "Polygon" or len(polys) != 1, "a feature of one polygon is a Polygon"
        out.append((f["properties"], [[[(float(x), float(y)) for x, y in ring] for ring in p] for p in polys]))
    return out, text


def shapefile_features(path):
    s, d = shp(path), V.dbf(path[:-4] + ".dbf")
    assert len(s["records"]) == d["nrecords"]
    return [({f[0]: v.decode().strip() for f, v in zip(d["fields"], row)}, rings(r)) for r, row in zip(s["records"], d["rows"])]


def area2(ring):
    """twice the signed area in map coordinates (y up): negative for a clockwise ring."""
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring[:-1], ring[1:]))
