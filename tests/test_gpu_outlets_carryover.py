"""bin/moveoutletstostrm carries every field of its outlet source over: a hand-made .dbf with N, F, C, D and L columns (tests/test_vector_layer.py)
next to a point shapefile goes in, and comes out with its descriptors and the bytes of every column unchanged, Dist_moved (N, width 6) appended and
the moved coordinates in the .shp; to GeoJSON the columns arrive by type.  The same from a GeoJSON source with properties to a shapefile."""
import os
import subprocess

import numpy as np
import pytest

import outlets_model as M
import taudem_amd as T
import vector_parse as V
from test_gpu_outlets import BIN, small_inputs, write_inputs
from test_vector_layer import bits, hand_made_dbf

pytestmark = pytest.mark.gpu


def run(f, src, out, md=3):
    r = subprocess.run([os.path.join(BIN, "moveoutletstostrm"), "-p", f("p.tif"), "-src", f("src.tif"), "-o", f(src), "-om", f(out), "-md", str(md)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_every_field_is_carried_over(ctx, tmp_path):
    g, i = small_inputs("checkerboard")
    f = write_inputs(tmp_path, i)
    n = len(i["ox"])
    T.write_points(f("gages.shp"), i["ox"], i["oy"], {})
    cols, rows = hand_made_dbf(f("gages.dbf"), n)
    before = V.dbf(f("gages.dbf"))
    c, r = M.to_cells(i["gt"], i["ox"], i["oy"])
    rx, ry, d = ctx.moveoutletstostrm(i["p"], i["src"], (c, r), 3, src_nodata=M.SRC_NODATA)
    cx, cy = M.cell_centre(i["gt"], rx, ry)
    want_x, want_y = np.where(d < 0, i["ox"], cx), np.where(d < 0, i["oy"], cy)
    assert (d > 0).any() and (d < 0).any()
    run(f, "gages.shp", "moved.shp")
    after, s = V.dbf(f("moved.dbf")), V.shp(f("moved.shp"))
    assert [fd[4] for fd in after["fields"][:-1]] == [fd[4] for fd in before["fields"]] and [row[:-1] for row in after["rows"]] == before["rows"] == rows
    assert after["fields"][-1][:4] == ("Dist_moved", "N", 6, 0) and [int(row[-1]) for row in after["rows"]] == d.tolist()
    assert bits([q[3] for q in s["records"]]) == bits(want_x) and bits([q[4] for q in s["records"]]) == bits(want_y)
    run(f, "gages.shp", "moved.geojson")
    pts, _ = V.geojson(f("moved.geojson"))
    assert [q[2]["GAGE_ID"] for q in pts] == [100 + k for k in range(n)] and [q[2]["NAME"] for q in pts] == ["st %d" % k for k in range(n)]
    assert [q[2]["Dist_moved"] for q in pts] == d.tolist() and bits([q[0] for q in pts]) == bits(want_x)
    # and back: the GeoJSON just written is an outlet source with properties of every type
    run(f, "moved.geojson", "again.shp")
    again = V.shapefile_points(f("again.shp"))
    names = [fd[:4] for fd in V.dbf(f("again.dbf"))["fields"]]
    assert names == [("GAGE_ID", "N", 9, 0), ("AREA_KM2", "N", 24, 15), ("NAME", "C", 80, 0), ("SINCE", "C", 80, 0), ("ACTIVE", "C", 80, 0), ("Dist_moved", "N", 9, 0),
                     ("Dist_moved", "N", 6, 0)]
    assert [float(q[2]["AREA_KM2"]) for q in again] == [1.5 * k for k in range(n)] and [q[2]["NAME"] for q in again] == ["st %d" % k for k in range(n)]
