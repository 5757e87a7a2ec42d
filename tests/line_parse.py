"""A reader and a writer of line shapefiles for the tests, written from the ESRI Shapefile Technical Description (July 1998) and calling nothing of the
product (tests/vector_parse.py reads the headers, the .shx and the .dbf):

    polylines(path)  -> dict: the header fields of vector_parse._header, records [(number, content words, shape type, box, parts [start...], points (n, 2))]
    build_shp(shape_type, lines, parts_of=None) -> bytes of a .shp of type 3, 13 or 23: per record the box, the parts, the points and, for 13 and 23, the
                        z range + z values and / or the m range + m values that those types carry (values that no reader should take for x or y)
    build_dbf(nrecords) -> bytes of a .dbf with one N(6) column ID holding 1, 2, ...
"""
import struct

import numpy as np

import vector_parse as V


def polylines(path):
    b = open(path, "rb").read()
    h = V._header(b)
    assert h["file_words"] * 2 == len(b), "the header's length is the file's"
    recs, pos = [], 100
    while pos < len(b):
        number, words = struct.unpack(">ii", b[pos:pos + 8])
        c = b[pos + 8:pos + 8 + 2 * words]
        t, = struct.unpack("<i", c[:4])
        box = struct.unpack("<4d", c[4:36])
        nparts, npoints = struct.unpack("<ii", c[36:44])
        parts = list(struct.unpack(f"<{nparts}i", c[44:44 + 4 * nparts]))
        pts = np.frombuffer(c[44 + 4 * nparts:44 + 4 * nparts + 16 * npoints], "<f8").reshape(npoints, 2)
        assert 44 + 4 * nparts + 16 * npoints == 2 * words, "a PolyLine record holds its box, parts and points and nothing else"
        recs.append((number, words, t, box, parts, pts, pos // 2))
        pos += 8 + 2 * words
    assert pos == len(b)
    h["records"] = recs
    return h


def build_shp(shape_type, lines, parts_of=None):
    body = b""
    allpts = np.concatenate([np.asarray(v, np.float64).reshape(-1, 2) for v in lines]) if lines else np.zeros((0, 2))
    for k, v in enumerate(lines):
        v = np.asarray(v, np.float64).reshape(-1, 2)
        parts = (parts_of or {}).get(k, [0])
        c = struct.pack("<i4d2i", shape_type, v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max(), len(parts), len(v))
        c += struct.pack(f"<{len(parts)}i", *parts) + v.astype("<f8").tobytes()
        if shape_type == 13:
            c += struct.pack("<2d", 777.0, 778.0) + np.full(len(v), 777.5, "<f8").tobytes()
        if shape_type in (13, 23):
            c += struct.pack("<2d", 888.0, 889.0) + np.full(len(v), 888.5, "<f8").tobytes()
        body += struct.pack(">ii", k + 1, len(c) // 2) + c
    box = (allpts[:, 0].min(), allpts[:, 1].min(), allpts[:, 0].max(), allpts[:, 1].max()) if len(allpts) else (0, 0, 0, 0)
    head = struct.pack(">i5ii", 9994, 0, 0, 0, 0, 0, (100 + len(body)) // 2) + struct.pack("<ii4d4d", 1000, shape_type, *box, 0, 0, 0, 0)
    return head + body


def build_dbf(n):
    d = struct.pack("<4BIHH20x", 3, 95, 7, 26, n, 32 + 32 + 1, 1 + 6)
    d += b"ID".ljust(11, b"\0") + b"N" + b"\0" * 4 + bytes([6, 0]) + b"\0" * 14 + b"\r"
    for i in range(n):
        d += b" " + str(i + 1).rjust(6).encode()
    return d + b"\x1a"
