"""Polygon layer files built byte by byte for the tests of the polygon reader: written from the ESRI Shapefile Technical Description (July 1998, shape
types 5, 15 and 25) and the dBASE III table layout, calling nothing of the product."""
import struct


def record(shape_type, rings):
    """The content of one record: rings is a list of point lists; None is a null shape.  Z (type 15) and M (15, 25) follow the points."""
    if rings is None:
        return struct.pack("<i", 0)
    pts = [p for r in rings for p in r]
    xs, ys = [p[0] for p in pts] or [0.0], [p[1] for p in pts] or [0.0]
    b = struct.pack("<i4dii", shape_type, min(xs), min(ys), max(xs), max(ys), len(rings), len(pts))
    first = 0
    for r in rings:
        b += struct.pack("<i", first)
        first += len(r)
    for x, y in pts:
        b += struct.pack("<2d", x, y)
    if shape_type == 15:
        b += struct.pack(f"<{2 + len(pts)}d", 0.0, 9.0, *[7.0 + k for k in range(len(pts))])
    if shape_type in (15, 25):
        b += struct.pack(f"<{2 + len(pts)}d", -1.0, 1.0, *[0.5] * len(pts))
    return b


def shp_bytes(shape_type, contents):
    """A .shp of the records' contents (bytes each)."""
    body = b"".join(struct.pack(">ii", k + 1, len(c) // 2) + c for k, c in enumerate(contents))
    head = struct.pack(">i5ii", 9994, 0, 0, 0, 0, 0, (100 + len(body)) // 2) + struct.pack("<ii8d", 1000, shape_type, *[0.0] * 8)
    return head + body


def dbf_bytes(field, texts, width=10, decimals=0, nrecords=None):
    """A .dbf of one N field; texts are written right-aligned as they are."""
    n = len(texts) if nrecords is None else nrecords
    head = struct.pack("<B3BIHH20x", 3, 95, 7, 26, n, 32 + 32 + 1, 1 + width)
    desc = field.encode().ljust(11, b"\0") + b"N" + b"\0" * 4 + bytes([width, decimals]) + b"\0" * 14
    return head + desc + b"\r" + b"".join(b" " + t.encode().rjust(width) for t in texts) + b"\x1a"


def write_layer(path, shape_type, features, field="ID", texts=None, **kw):
    """path.shp and path.dbf of features (ring lists, None for a null shape); the field holds 1, 2, ... unless texts are given."""
    open(path, "wb").write(shp_bytes(shape_type, [record(shape_type, f) for f in features]))
    open(path[:-4] + ".dbf", "wb").write(dbf_bytes(field, texts if texts is not None else [str(k + 1) for k in range(len(features))], **kw))
    return path


def text_of(features, values=None):
    """What tests/regiongrid/reader_main.cpp prints for a layer: features as ring lists."""
    out = []
    for i, rings in enumerate(features):
        out.append(f"feature {i} {len(rings)} {values[i] if values is not None else '-'}")
        out += ["ring" + "".join(" %.17g %.17g" % (x, y) for x, y in r) for r in rings]
    return "".join(line + "\n" for line in out)
