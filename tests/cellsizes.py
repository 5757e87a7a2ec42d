"""Per-row cell sizes (dxc[j], dyc[j]) that actually vary from row to row.

Every tool takes its cell size per row; for a geographic raster the sizes follow each row's latitude (the reference's tiffIO
constructor, mirrored by geotiff.cpp).  With constant sizes a kernel that reads the wrong row's geometry - donor row for the
receiver's, tile-local for array row, a halo off by one, strip-local for global - changes no bit; with these rows it does.

    geographic_rows(ny, lat_top, dlat, dlon)  the sizes the product's own GeoTIFF reader derives for a geographic raster
    wild_rows(ny, seed)                       independent, non-monotone dx and dy per row (dx / dy between 0.2 and 5; some rows dx == dy)
"""
import os
import tempfile

import numpy as np

KINDS = ("fine", "band", "wild")


def geographic_rows(ny, lat_top, dlat, dlon):
    """(dxc, dyc) in metres of a geographic raster of ny rows whose top edge is at lat_top: written as a small GeoTIFF flagged
    geographic and read back, so the values come from the product's reader (pinned to the reference by the `geographic` golden).
    A band that crosses the pole or the equator is not what this is for: the rows must stay within (-90, 90)."""
    import taudem_amd as T

    assert -90.0 < lat_top - ny * dlat and lat_top < 90.0, "rows must stay within (-90, 90) degrees"
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rows.tif")
        T.write_raster(path, np.zeros((ny, 2), np.float32), -9999.0, geotransform=(10.0, dlon, 0.0, lat_top, 0.0, -dlat), geographic=True)
        _, info = T.read_raster(path, np.float32)
    return np.ascontiguousarray(info["dxc"], dtype=np.float64), np.ascontiguousarray(info["dyc"], dtype=np.float64)


def wild_rows(ny, seed):
    """(dxc, dyc): a random dy around 25 m per row and dx = dy * r with log(r) uniform in [log 0.2, log 5], both independent from row
    to row, so that a row mix-up flips D8 directions and D-infinity facets, not just low bits.  Every 7th row has dx == dy exactly
    (the diagonal band of the facet comparison), and every 11th row repeats the previous row's sizes (ties between rows)."""
    rng = np.random.default_rng(4000 + seed)
    dy = 25.0 * np.exp(rng.uniform(-0.7, 0.7, ny))
    r = np.exp(rng.uniform(np.log(0.2), np.log(5.0), ny))
    dx = dy * r
    j = np.arange(ny)
    dx[j % 7 == 3] = dy[j % 7 == 3]
    rep = (j % 11 == 5) & (j > 0)
    dx[rep], dy[rep] = dx[np.flatnonzero(rep) - 1], dy[np.flatnonzero(rep) - 1]
    return np.ascontiguousarray(dx), np.ascontiguousarray(dy)


def rows(kind, ny, seed=0):
    """(dxc, dyc) of one of KINDS for ny rows:
        fine  mid-latitude 1 arc-second cells from 45.3 N down (about 22 x 31 m, dx shrinking slowly to the north)
        band  square degrees cells covering 70 N -> 40 N whatever ny is (0.01 degree at 3000 rows): dx / dy runs from 0.34 to 0.77
        wild  wild_rows(ny, seed)"""
    if kind == "fine":
        return geographic_rows(ny, 45.3, 1.0 / 3600.0, 1.0 / 3600.0)
    if kind == "band":
        return geographic_rows(ny, 70.0, 30.0 / ny, 30.0 / ny)
    if kind == "wild":
        return wild_rows(ny, seed)
    raise ValueError(kind)
