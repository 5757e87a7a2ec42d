"""The stream network layer and CatchOutlets restated in Python, and what the records of tests/golden/netlayer_<case>.npz look like
(tests/golden/make_golden_netlayer.py runs the real tools).

    net_rows(tree, coord, geographic)        reachshape() (src/streamnet.cpp:244-365) per link: the 17 fields {name: list} and the reversed vertex lists
    catch_outlets(fields, lines, p, gt, ...)  catchoutlets() / CheckPoint() (src/CatchOutlets.cpp:87-368): the outlets [(x, y, {field: value})] in order
    parse_lines(text), parse_points(text)    the records of tests/streamnet/ogr_record_lines_stub.h and tests/netlayer/ogr_replay_lines_stub.h
    rows_of_text(tree bytes, coord bytes)    the rows of the -tree / -coord files, values as the text holds them
    grid(fields)                             the (mindist, minarea, gwstartno) runs of a network, from its own lengths and areas

The arithmetic is the reference's: double throughout, but the distance, elevation and area columns are floats, drop is a float difference and the
three DOUT values are floats.  geo_to_length is tiffIO::geotoLength (src/tiffIO.cpp:434-445) on the host libm, through Python's math module.
"""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
INT_FIELDS = ("LINKNO", "DSLINKNO", "USLINKNO1", "USLINKNO2", "DSNODEID", "strmOrder", "Magnitude", "WSNO")
REAL_FIELDS = ("Length", "DSContArea", "strmDrop", "Slope", "StraightL", "USContArea", "DOUTEND", "DOUTSTART", "DOUTMID")
FIELDS = ("LINKNO", "DSLINKNO", "USLINKNO1", "USLINKNO2", "DSNODEID", "strmOrder", "Length", "Magnitude", "DSContArea", "strmDrop", "Slope", "StraightL",
          "USContArea", "WSNO", "DOUTEND", "DOUTSTART", "DOUTMID")
TREE_COLUMN = {"LINKNO": 0, "DSLINKNO": 3, "USLINKNO1": 4, "USLINKNO2": 5, "DSNODEID": 7, "strmOrder": 6, "Magnitude": 8, "WSNO": 0}
OUT_FIELDS = ("LINKNO", "DSLINKNO", "USLINKNO1", "USLINKNO2", "DOUTEND", "Id")
VARIANTS = ("plain", "outlets")
PI, ELIPA, ELIPB = 3.14159265359, 6378137.000, 6356752.314
BOA = ELIPB / ELIPA
D1 = (-99, 0, -1, -1, -1, 0, 1, 1, 1)   # row steps
D2 = (-99, 1, 1, 0, -1, -1, -1, 0, 1)   # column steps


def geo_to_length(dlon, dlat, lat):
    dlat = dlat * PI / 180.
    dlon = dlon * PI / 180.
    lat = lat * PI / 180.
    beta = math.atan(BOA * math.tan(lat))
    dbeta = dlat * BOA * (math.cos(beta) / math.cos(lat)) * (math.cos(beta) / math.cos(lat))
    a, b = ELIPA * math.sin(beta), ELIPB * math.cos(beta)
    ds2 = (a * a + b * b) * (dbeta * dbeta)   # pow(., 2) is the exact square rounded once, like the product
    return ELIPA * math.cos(beta) * abs(dlon), math.sqrt(ds2)


def _step(dx, dy, y, geographic):
    if geographic:
        dx, dy = geo_to_length(dx, dy, y)
    return math.sqrt(dx * dx + dy * dy)


def net_rows(tree, coord, geographic):
    tree = np.asarray(tree, np.int64).reshape(-1, 9)
    coord = np.asarray(coord, np.float64).reshape(-1, 5)
    fields, lines = {k: [] for k in FIELDS}, []
    for t in tree:
        c = coord[int(t[1]):int(t[2]) + 1]
        npnt = len(c)
        lengthd, elev, area = (c[:, k].astype(np.float32) for k in (2, 3, 4))
        x1, y1 = float(c[0, 0]), float(c[0, 1])
        x, y, xlast, ylast, length = x1, y1, x1, y1, 0.0
        usarea = float(area[0])
        dslast = dsarea = usarea
        for j in range(npnt):
            x, y = float(c[j, 0]), float(c[j, 1])
            dl = _step(x - xlast, y - ylast, y, geographic)
            if dl > 0.:
                length = length + dl
                xlast, ylast = x, y
                dsarea = dslast
                dslast = float(area[j])
        drop = float(np.float32(elev[0] - elev[npnt - 1]))
        dsdist, usdist = lengthd[npnt - 1], lengthd[0]
        middist = np.float32(float(np.float32(dsdist + usdist)) * 0.5)
        slope = drop / length if length > 0. else 0.
        glength = _step(x - x1, y - y1, y, geographic)
        for k, col in TREE_COLUMN.items():
            fields[k].append(int(np.int32(t[col])))
        for k, v in zip(REAL_FIELDS, (length, dsarea, drop, slope, glength, usarea, float(dsdist), float(usdist), float(middist))):
            fields[k].append(v)
        lines.append(c[::-1, :2].copy())
    return fields, lines


def catch_outlets(fields, lines, p, gt, mindist, minarea, gwstartno, seen=None):
    """p: the int16 raster; gt: GDAL's six numbers.  The reference's recursion, with a stack of its own.  seen (a dict, optional) counts what a run met:
    "mindist" links not written for their distance alone, "minarea" links whose subtree was cut, "bad_p" outlet links whose down end has no direction,
    "stays" down ends whose step would leave the raster."""
    seen = {} if seen is None else seen
    for k in ("mindist", "minarea", "bad_p", "stays"):
        seen.setdefault(k, 0)
    ny, nx = p.shape
    x0, dlon, y0, dlat = gt[0], abs(gt[1]), gt[3], abs(gt[5])
    n = len(lines)
    kept = [i for i in range(n) if fields["DSLINKNO"][i] < 0 or fields["USLINKNO1"][i] >= 0 or fields["USLINKNO2"][i] >= 0]
    at = {}
    for i in kept:
        at.setdefault(int(fields["LINKNO"][i]), i)
    shown = lambda i: float(fields["DOUTEND"][i] if fields["DSLINKNO"][i] < 0 else fields["DOUTSTART"][i])  # noqa: E731
    point = lambda i: lines[i][0] if fields["DSLINKNO"][i] < 0 else lines[i][-1]  # noqa: E731
    out, gw = [], int(gwstartno)

    def write(i, x, y):
        nonlocal gw
        out.append((float(x), float(y), {"LINKNO": int(fields["LINKNO"][i]), "DSLINKNO": int(fields["DSLINKNO"][i]), "USLINKNO1": int(fields["USLINKNO1"][i]),
                                         "USLINKNO2": int(fields["USLINKNO2"][i]), "DOUTEND": shown(i), "Id": gw}))
        gw += 1

    for i in kept:
        if fields["DSLINKNO"][i] >= 0:
            continue
        px, py = point(i)
        gx, gy = int((px - x0) / dlon), int((y0 - py) / dlat)   # int(): truncation towards zero, as (int) in C
        if not (0 <= gx < nx and 0 <= gy < ny):
            continue
        d = int(p[gy, gx])
        if not 1 <= d <= 8:
            seen["bad_p"] += 1
            continue
        tx, ty = gx + D2[d], gy + D1[d]
        if not (0 <= tx < nx and 0 <= ty < ny):
            tx, ty = gx, gy
            seen["stays"] += 1
        write(i, x0 + dlon / 2. + tx * dlon, y0 - dlat / 2. - ty * dlat)
        stack = [(int(fields["USLINKNO2"][i]), 0.0), (int(fields["USLINKNO1"][i]), 0.0)]
        while stack:
            link, downout = stack.pop()
            if link < 0 or link not in at:
                continue
            q = at[link]
            big = float(fields["USContArea"][q]) > minarea
            if shown(q) - downout > mindist and big:
                write(q, *point(q))
                downout = shown(q)
            elif big:
                seen["mindist"] += 1
            if big:
                stack += [(int(fields["USLINKNO2"][q]), downout), (int(fields["USLINKNO1"][q]), downout)]
            elif fields["USLINKNO1"][q] >= 0 or fields["USLINKNO2"][q] >= 0:
                seen["minarea"] += 1
    return out


def parse_lines(text):
    """fields {name: list of int / float}, lines [(vertices, 2) array] of a line record"""
    fields, lines = {}, []
    for ln in text.splitlines():
        w = ln.split()
        npnt = int(w[0])
        lines.append(np.array([float(v) for v in w[1:1 + 2 * npnt]], np.float64).reshape(npnt, 2))
        for tok in w[1 + 2 * npnt:]:
            k, v = tok.split("=")
            fields.setdefault(k, []).append(int(v) if k in INT_FIELDS else float(v))
    return fields, lines


def parse_points(text):
    out = []
    for ln in text.splitlines():
        w = ln.split()
        f = dict(tok.split("=") for tok in w[2:])
        out.append((float(w[0]), float(w[1]), {k: (float(v) if k == "DOUTEND" else int(v)) for k, v in f.items()}))
    return out


def rows_of_text(tree_bytes, coord_bytes):
    tree = np.array([[int(v) for v in ln.split()] for ln in bytes(tree_bytes).decode().splitlines()], np.int64).reshape(-1, 9)
    coord = np.array([[float(v) for v in ln.split()] for ln in bytes(coord_bytes).decode().splitlines()], np.float64).reshape(-1, 5)
    return tree, coord


def same_layer(a, b):
    """two (fields, lines): equal integers, bit-equal reals and vertices"""
    fa, la = a
    fb, lb = b
    if len(la) != len(lb) or set(fa) != set(fb):
        return False
    if any(x.shape != y.shape or x.tobytes() != y.tobytes() for x, y in zip(la, lb)):
        return False
    for k in fa:
        va, vb = (np.asarray(v, np.int64 if k in INT_FIELDS else np.float64) for v in (fa[k], fb[k]))
        if va.shape != vb.shape or va.tobytes() != vb.tobytes():
            return False
    return True


def grid(fields):
    """[(mindist, minarea, gwstartno)]: nothing held back; a distance above which half of the links lie; an area a third of the links do not reach, with
    another first Id; both"""
    if not fields or not fields.get("Length"):
        return [(0.0, 0.0, 1), (25.0, 0.0, 1), (0.0, 30.0, 7), (25.0, 30.0, 1)]
    d = sorted(v for v in fields["Length"] if v > 0) or [1.0]
    a = sorted(fields["USContArea"])
    md, ma = float(d[len(d) // 2]) * 1.5, float(a[len(a) // 3])
    return [(0.0, 0.0, 1), (md, 0.0, 1), (0.0, ma, 7), (md, ma, 1)]


def load(name):
    g = np.load(os.path.join(HERE, "golden", f"netlayer_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def text(a):
    return bytes(a).decode()
