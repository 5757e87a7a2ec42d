"""A reader of point layers for the tests, written from the format descriptions (ESRI Shapefile Technical Description, July 1998; the dBASE III
table layout; RFC 7946) and calling nothing of the product: what the product's writer wrote is read back through other code.

    shp(path)      -> dict: file_code, file_words, version, shape_type, bbox (xmin, ymin, xmax, ymax), zm (four doubles), records [(number, words, type, x, y)]
    shx(path)      -> dict: the same header fields, index [(offset in words, content words)]
    dbf(path)      -> dict: version, nrecords, header_bytes, record_bytes, fields [(name, type letter, width, decimals, the 32 descriptor bytes)],
                      rows [[bytes per field]], deleted [flag byte per record], terminator, eof
    geojson(path)  -> [(x, y, {property: value})] with json.loads, and the text for digit checks
    shapefile_points(path) -> [(x, y, {field: stripped text})] of a .shp and its .dbf
"""
import json
import struct


def _header(b):
    assert len(b) >= 100
    code, = struct.unpack(">i", b[0:4])
    words, = struct.unpack(">i", b[24:28])
    version, shape_type = struct.unpack("<ii", b[28:36])
    box = struct.unpack("<4d", b[36:68])
    zm = struct.unpack("<4d", b[68:100])
    return dict(file_code=code, unused=b[4:24], file_words=words, version=version, shape_type=shape_type, bbox=box, zm=zm)


def shp(path):
    b = open(path, "rb").read()
    h = _header(b)
    assert h["file_words"] * 2 == len(b), "the header's length is the file's"
    recs, pos = [], 100
    while pos < len(b):
        number, words = struct.unpack(">ii", b[pos:pos + 8])
        t, = struct.unpack("<i", b[pos + 8:pos + 12])
        x, y = struct.unpack("<2d", b[pos + 12:pos + 28])
        recs.append((number, words, t, x, y, pos // 2))
        pos += 8 + 2 * words
    assert pos == len(b)
    h["records"] = recs
    return h


def shx(path):
    b = open(path, "rb").read()
    h = _header(b)
    assert h["file_words"] * 2 == len(b) and (len(b) - 100) % 8 == 0
    h["index"] = [struct.unpack(">ii", b[p:p + 8]) for p in range(100, len(b), 8)]
    return h


def dbf(path):
    b = open(path, "rb").read()
    version, yy, mm, dd, nrec, hlen, rlen = struct.unpack("<4BIHH", b[:12])
    fields, pos = [], 32
    while b[pos] != 0x0D:
        d = b[pos:pos + 32]
        fields.append((d[:11].split(b"\0")[0].decode(), chr(d[11]), d[16], d[17], d))
        pos += 32
    assert pos + 1 == hlen and rlen == 1 + sum(f[2] for f in fields)
    rows, deleted = [], []
    for i in range(nrec):
        r = b[hlen + i * rlen:hlen + (i + 1) * rlen]
        assert len(r) == rlen
        deleted.append(r[:1])
        o, row = 1, []
        for f in fields:
            row.append(r[o:o + f[2]])
            o += f[2]
        rows.append(row)
    tail = b[hlen + nrec * rlen:]
    return dict(version=version, date=(yy, mm, dd), nrecords=nrec, header_bytes=hlen, record_bytes=rlen, fields=fields, rows=rows, deleted=deleted, terminator=b[pos], eof=tail)


def geojson(path):
    text = open(path).read()
    doc = json.loads(text)
    assert doc["type"] == "FeatureCollection"
    out = []
    for f in doc["features"]:
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Point"
        x, y = f["geometry"]["coordinates"]
        out.append((float(x), float(y), f["properties"]))
    return out, text


def shapefile_points(path):
    """[(x, y, {field: stripped text})] of path.shp + .dbf"""
    s, d = shp(path), dbf(path[:-4] + ".dbf")
    assert len(s["records"]) == d["nrecords"]
    return [(r[3], r[4], {f[0]: v.decode().strip() for f, v in zip(d["fields"], row)}) for r, row in zip(s["records"], d["rows"])]
