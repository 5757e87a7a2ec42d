"""EditRaster (src/EditRaster.cpp:69-168) restated in numpy, the change-file scanner restated in Python, and the small rasters and change files of
tests/golden/editraster_small.npz, which tests/golden/make_golden_editraster.py runs the real tool on.

    cells(x, y, gt)                      tiffIO::geoToGlobalXY: (int) truncation towards zero of (x - xleft) / dx and (ytop - y) / dy
    scan_changes(text)                   the records "%lf,%lf,%d" scans after the first line, up to the first one that does not scan
    edit(raster, nodata, cols, rows, vals)   the output raster: nodata -> -32768, then the changes on the raster in list order (the last one of a cell holds)
    process_lines(...)                   the "Process: 0 changing" lines of the tool, one per change on the raster in file order
"""
import re

import numpy as np

OUT_NODATA = np.int16(-32768)
DX = 30.0


def geotransform(ny):
    return (1000.0, DX, 0.0, 5000.0 + DX * ny, 0.0, -DX)


def cells(x, y, gt):
    """columns, rows (int64) as C's (int) conversion gives them: truncation towards zero, so a point less than one cell left of or above the raster lands in
    column / row 0"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.trunc((x - gt[0]) / gt[1]).astype(np.int64), np.trunc((gt[3] - y) / -gt[5]).astype(np.int64)


_NUM = r"[ \t\n\r\f\v]*([+-]?(?:[0-9]+\.?[0-9]*(?:[eE][+-]?[0-9]+)?|\.[0-9]+(?:[eE][+-]?[0-9]+)?))"
_INT = r"[ \t\n\r\f\v]*([+-]?[0-9]+)"
_RECORD = re.compile(_NUM + "," + _NUM + "," + _INT)


def scan_changes(text):
    """x, y (float64), vals (int64; a value beyond int16 is the caller's to judge) of a change file's text.  Plain decimal numbers only: what the fixtures hold."""
    nl = text.find("\n")
    rest = "" if nl < 0 else text[nl + 1:]
    xs, ys, vs, pos = [], [], [], 0
    while True:
        m = _RECORD.match(rest, pos)
        if not m:
            break
        xs.append(float(m.group(1))); ys.append(float(m.group(2))); vs.append(int(m.group(3)))
        pos = m.end()
    return np.array(xs, np.float64), np.array(ys, np.float64), np.array(vs, np.int64)


def edit(raster, nodata, cols, rows, vals):
    ny, nx = raster.shape
    out = np.where(raster == np.int16(nodata), OUT_NODATA, raster).astype(np.int16)
    for c, r, v in zip(np.asarray(cols, np.int64), np.asarray(rows, np.int64), np.asarray(vals, np.int64)):
        if 0 <= c < nx and 0 <= r < ny:
            out[r, c] = np.int16(v)
    return out


def process_lines(x, y, vals, gt, shape, as_reference=False):
    """as_reference: the reference scans "%d" into a short that lies next to its `rank` on the stack, so the upper half of a scanned value lands in rank's
    lower half: after a negative value it says "Process: 65535" (and, if that was the last record, keeps its "Compute time" line to itself, being no
    longer rank 0).  The project prints rank 0 always."""
    ny, nx = shape
    c, r = cells(x, y, gt)
    return ["Process: %d changing %f, %f, %d" % (65535 if as_reference and v < 0 else 0, a, b, v)
            for a, b, v, ci, ri in zip(x, y, vals, c, r) if 0 <= ci < nx and 0 <= ri < ny]


def _raster(ny, nx, nodata, holes, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 9, size=(ny, nx)).astype(np.int16)
    for r, c in holes:
        a[r, c] = nodata
    return a


def cases():
    """name -> (raster int16, nodata, {change file name: text})"""
    out = {}
    for name, ny, nx, nodata, holes in (("one", 1, 1, -32768, ()), ("small", 3, 4, -1, ((0, 1), (2, 3), (1, 0))), ("wide", 5, 67, 0, ((0, 0), (4, 66), (2, 33)))):
        a = _raster(ny, nx, nodata, holes, 7000 + nx)
        if name == "wide":
            a[3, 5:60] = 0   # a run of nodata cells across 16-byte groups
        x0, _, _, y0, _, _ = geotransform(ny)
        xr, yb = x0 + DX * nx, y0 - DX * ny                     # the right and bottom edges
        xm, ym = x0 + DX * (nx - 0.5), y0 - DX * (ny - 0.5)     # the centre of the last cell
        files = {
            "none": "x,y,value\n",
            "dup": "x,y,value\n%r,%r,11\n%r,%r,12\n%r,%r,13\n" % (xm, ym, x0 + 1.0, y0 - 1.0, xm, ym),
            # on the left and top edges; less than a cell left of and above the raster; on the right and the bottom edge; far off
            "edges": "any header, not looked at\n%r,%r,21\n%r,%r,22\n%r,%r,23\n%r,%r,24\n%r,%r,25\n%r,%r,26\n"
                     % (x0, y0, x0 - 10.0, ym, xm, y0 + 29.0, xr, ym, xm, yb, x0 - 31.0, y0 + 31.0),
            "malformed": "x,y,value\n%r,%r,31\n%r;%r;32\n%r,%r,33\n" % (xm, ym, x0 + 1.0, y0 - 1.0, x0 + 1.0, y0 - 1.0),
            # the extremes of int16, and white space where the scanner takes it: before a number, not before a comma
            "values": "x,y,value\n%r,%r,-32768\n  %r,  %r,\n 32767\n%r,%r,-5\n" % (x0 + 1.0, y0 - 1.0, xm, ym, x0 + 1.0, y0 - 1.0),
        }
        out[name] = (a, nodata, files)
    return out
