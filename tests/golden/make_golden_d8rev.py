"""Golden vectors for D8HDistToStrm (src/D8HDistToStrm.cpp) and GageWatershed (src/gagewatershed.cpp): runs the REAL reference tools on the
D8 directions of the committed cases.  Build container only, after build() has left the reference's common objects in oracle/_ref/obj:

    python tests/golden/make_golden_d8rev.py

The reference tools are compiled into a temporary directory (the flags of oracle/Makefile's REFFLAGS, linked against oracle/_ref/obj);
nothing is written under oracle/.  d8rev_<case>.npz holds
  * the inputs: p with a few p == 0 cells, a few nodata cells under stream cells and a 2-cell cycle; src = ad8 >= 20 as int16 (0 / 1, with
    nodata holes); ad8 as an int32 contributing-area raster (nodata -1); per-row cell sizes; the geotransform of the files;
  * dist_src: d8hdisttostrm -src src (default -thresh 1), dist_ad8: -src ad8 -thresh 40;
  * outlets (text file `x y id`, non-sequential ids): on the largest-area cell of the rows a 3-rank split cuts, a gauge five steps
    upstream of another, two outlets on one cell, one off the raster; their columns / rows (geoToGlobalXY) and ids;
  * gw and id_text: gagewatershed -gw / -id.
The reference's 3-rank runs are compared with its 1-rank runs on `holes`, `plain` and `geographic` (they agree).  The files are named
d8rev_*.npz, not case_*.npz: conftest.golden_cases() takes every case_*.npz as a case.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import d8rev_model as M  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
MPI_ROOT = "/opt/conda"
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
CASES = ("plain", "holes", "rect_dxdy", "geographic", "fourway_mask")
DX_ = (0, 1, 1, 0, -1, -1, -1, 0, 1)
DY_ = (0, 0, -1, -1, -1, 0, 1, 1, 1)


def build_tool(d, name, sources):
    """Compiles reference sources into directory d; returns the executable."""
    inc = ["-Igdal_shim", f"-I{os.path.join(ROOT, 'oracle', '_ref', 'mpiinc')}", f"-I{REF_SRC}"]
    flags = ["-std=c++17", "-O3", "-w"]   # oracle/Makefile REFFLAGS
    objs = []
    for s in sources:
        o = os.path.join(d, s + ".o")
        subprocess.run(["g++"] + flags + inc + ["-c", os.path.join(REF_SRC, s + ".cpp"), "-o", o], check=True, cwd=os.path.join(ROOT, "oracle"))
        objs.append(o)
    common = [os.path.join(OBJ, f + ".o") for f in ("commonLib", "tiffIO", "ReadOutlets", "shim", "geotiff", "outlets")]
    exe = os.path.join(d, name)
    subprocess.run(["g++"] + objs + common + [f"{MPI_ROOT}/lib/libmpi.so", f"-Wl,-rpath,/usr/lib/x86_64-linux-gnu:{MPI_ROOT}/lib", "-Wl,--allow-shlib-undefined",
                                              "-lz", "-o", exe], check=True)
    return exe


def inputs(name):
    g = np.load(os.path.join(OUT, f"case_{name}.npz"))
    p = g["p"].copy()
    ad8 = g["ad8"]
    ny, nx = p.shape
    rng = np.random.default_rng(4100 + nx + ny)
    stream = (ad8 >= 20) & (p != M.P_NODATA)
    src = np.where(stream, 1, 0).astype(np.int16)
    src[ad8 < -0.5] = M.SRC_NODATA
    inner = np.zeros((ny, nx), bool)
    inner[2:-2, 2:-2] = True
    cand = np.flatnonzero(inner & ~stream & (p > 0))
    zero = rng.choice(cand, 6, replace=False)
    p.flat[zero] = 0                                                    # p == 0: counted at k = 4, never a result
    scells = np.flatnonzero(inner & stream)
    p.flat[rng.choice(scells, 4, replace=False)] = M.P_NODATA            # stream cells without a direction: still sources
    cand = np.flatnonzero(inner & ~stream & (p > 0))
    rng.shuffle(cand)
    for c in cand:                                                      # a 2-cell cycle: c -> east neighbour -> c
        if not stream.flat[c + 1] and p.flat[c + 1] > 0:
            p.flat[c], p.flat[c + 1] = 1, 5
            break
    holes = np.flatnonzero(rng.random(ny * nx) < 0.006)
    src.flat[holes] = M.SRC_NODATA                                      # src nodata holes: not stream cells
    ad8i = np.where(ad8 < -0.5, -1, np.rint(ad8)).astype(np.int32)       # contributing area (cells) as a LONG raster
    return g, p, src, ad8i


def outlets(p, ad8i):
    """(cols, rows, ids): largest-area cells of the cut rows of a 3-rank split and of two more rows, a gauge five steps upstream of
    another, a second outlet on one cell, one off the raster."""
    ny, nx = p.shape
    base = ny // 3
    rows = [base - 1, base, 2 * base - 1, 2 * base, ny // 2 + 3, ny - 4]
    cols = [int(np.argmax(np.where(p[r] > 0, ad8i[r], -1))) for r in rows]
    x, y = cols[-1], rows[-1]                                           # follow the flow five steps down from the last one
    for _ in range(5):
        k = int(p[y, x])
        if not 1 <= k <= 8 or not (0 <= x + DX_[k] < nx and 0 <= y + DY_[k] < ny):
            break
        x, y = x + DX_[k], y + DY_[k]
    cols.append(x)
    rows.append(y)
    cols.append(cols[2])                                                # a second outlet on one cell: not placed, not in the -id file
    rows.append(rows[2])
    cols.append(nx + 7)                                                 # off the raster
    rows.append(ny // 2)
    ids = [17, 3, 250, 42, 9001, 5, 64, 1234, 77]
    return np.array(cols, np.int32), np.array(rows, np.int32), np.array(ids, np.int32)


def make(exes, name, check_ranks=0):
    g, p, src, ad8i = inputs(name)
    ny, nx = p.shape
    dx, dy, geographic = float(g["dx"]), float(g["dy"]), bool(g["geographic"])
    gt = (-111.9, dx, 0.0, 41.9, 0.0, -dy) if geographic else (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)
    cols, rows, ids = outlets(p, ad8i)
    res = {"p": p, "src": src.astype(np.int32), "src_nodata": np.int32(M.SRC_NODATA), "ad8": ad8i, "ad8_nodata": np.int32(-1), "dxc": g["dxc"],
           "dyc": g["dyc"], "gt": np.array(gt), "geographic": np.bool_(geographic), "cols": cols, "rows": rows, "ids": ids}
    agree = []
    with tempfile.TemporaryDirectory() as d:
        f = lambda s: os.path.join(d, s)  # noqa: E731
        T.write_raster(f("p.tif"), p, M.P_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("src.tif"), src, M.SRC_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("ad8.tif"), ad8i, -1, geotransform=gt, geographic=geographic)
        with open(f("gauges.txt"), "w") as fo:
            for c, r, i in zip(cols, rows, ids):
                fo.write(f"{float(gt[0] + (c + 0.5) * dx)!r} {float(gt[3] - (r + 0.5) * dy)!r} {i}\n")
        runs = {"dist_src": ["-src", f("src.tif")], "dist_ad8": ["-src", f("ad8.tif"), "-thresh", str(M.THRESH_AD8)]}
        for key, extra in runs.items():
            O.run_ref(exes["dist"], ["-p", f("p.tif")] + extra + ["-dist", f(key + ".tif")])
            res[key], _ = T.read_raster(f(key + ".tif"))
            if check_ranks:
                O.run_ref(exes["dist"], ["-p", f("p.tif")] + extra + ["-dist", f(key + "3.tif")], check_ranks)
                a3, _ = T.read_raster(f(key + "3.tif"))
                agree.append((key, bool(np.array_equal(a3.view(np.uint32), res[key].view(np.uint32)))))
        O.run_ref(exes["gage"], ["-p", f("p.tif"), "-o", f("gauges.txt"), "-gw", f("gw.tif"), "-id", f("id.txt")])
        res["gw"], _ = T.read_raster(f("gw.tif"), np.int32)
        res["id_text"] = np.array(open(f("id.txt")).read())
        if check_ranks:
            O.run_ref(exes["gage"], ["-p", f("p.tif"), "-o", f("gauges.txt"), "-gw", f("gw3.tif"), "-id", f("id3.txt")], check_ranks)
            a3, _ = T.read_raster(f("gw3.tif"), np.int32)
            agree.append(("gw", bool(np.array_equal(a3, res["gw"]))))
            agree.append(("id", open(f("id3.txt")).read() == str(res["id_text"])))
    np.savez_compressed(os.path.join(OUT, f"d8rev_{name}.npz"), **res)
    v = res["dist_src"]
    print(name, p.shape, "dist max", float(v[v > -1e30].max()), "nodata", int((v < -1e30).sum()), "gw labels", np.unique(res["gw"]).size)
    print(str(res["id_text"]))
    if agree:
        print(f"  {check_ranks} ranks vs 1 rank:", "; ".join(f"{k}: {'same' if a else 'DIFFERENT'}" for k, a in agree))
        assert all(a for _, a in agree), "the reference's multi-rank run differs from its 1-rank run"


if __name__ == "__main__":
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exes = {"dist": build_tool(tmp, "d8hdisttostrm", ("D8HDistToStrm", "D8HDistToStrmmn")),
                "gage": build_tool(tmp, "gagewatershed", ("gagewatershed", "gagewatershedmn"))}
        for c in CASES:
            make(exes, c, check_ranks=3 if c in ("holes", "plain", "geographic") else 0)
