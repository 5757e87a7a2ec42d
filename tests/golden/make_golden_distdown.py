"""Golden vectors for DinfDistDown (src/DinfDistDown.cpp): runs the REAL reference tool on the D-infinity angles and pit-filled
elevations of the committed cases.  Build container only, after build() has left the reference's common objects in oracle/_ref/obj:

    python tests/golden/make_golden_distdown.py

The reference tool is compiled into a temporary directory (the flags of oracle/Makefile's REFFLAGS, linked against oracle/_ref/obj);
nothing is written under oracle/.  distdown_<case>.npz holds the inputs (ang with one stream cell without an angle, fel with a few
nodata cells, src = sca above a threshold with a few nodata cells, weights with a few nodata cells, per-row cell sizes) and, for
every -m combination, the reference's raster with the default contamination check (dd_<stat>_<type>), with -nc (..._nc) and with
-wg (..._wg).  The files are named distdown_*.npz, not case_*.npz: conftest.golden_cases() takes every case_*.npz as a case.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
MPI_ROOT = "/opt/conda"
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
STATS = ("ave", "max", "min")
KINDS = ("h", "v", "p", "s")
CASES = ("plain", "holes", "rect_dxdy", "geographic", "fourway_mask")
SRC_NODATA = -32768


def build_tool(d):
    """Compiles the reference's DinfDistDown into directory d; returns the executable."""
    inc = ["-Igdal_shim", f"-I{os.path.join(ROOT, 'oracle', '_ref', 'mpiinc')}", f"-I{REF_SRC}"]
    flags = ["-std=c++17", "-O3", "-w"]   # oracle/Makefile REFFLAGS
    objs = []
    for s in ("DinfDistDown", "DinfDistDownmn"):
        o = os.path.join(d, s + ".o")
        subprocess.run(["g++"] + flags + inc + ["-c", os.path.join(REF_SRC, s + ".cpp"), "-o", o], check=True, cwd=os.path.join(ROOT, "oracle"))
        objs.append(o)
    common = [os.path.join(OBJ, f + ".o") for f in ("commonLib", "tiffIO", "ReadOutlets", "shim", "geotiff", "outlets")]
    exe = os.path.join(d, "dinfdistdown")
    subprocess.run(["g++"] + objs + common + [f"{MPI_ROOT}/lib/libmpi.so", f"-Wl,-rpath,/usr/lib/x86_64-linux-gnu:{MPI_ROOT}/lib", "-Wl,--allow-shlib-undefined",
                                              "-lz", "-o", exe], check=True)
    return exe


def inputs(name):
    g = np.load(os.path.join(OUT, f"case_{name}.npz"))
    ang = g["ang"].copy()
    fel = g["fel"].copy()
    ny, nx = ang.shape
    rng = np.random.default_rng(700 + nx + ny)
    sca = g["sca"]
    valid = sca > -1e30
    thr = np.quantile(sca[valid], 0.9)
    src = np.where(valid & (sca >= thr), 1, 0).astype(np.int16)
    src[(rng.random((ny, nx)) < 0.01) & (src == 0)] = 2                       # isolated stream cells (any value >= 1)
    src[rng.random((ny, nx)) < 0.01] = SRC_NODATA                              # nodata src: not a stream cell
    sy, sx = np.argwhere(src >= 1)[len(np.argwhere(src >= 1)) // 2]
    ang[sy, sx] = -3.402823466e38                                              # a stream cell without an angle: never queued, stays nodata
    felnd = rng.random((ny, nx)) < 0.004
    fel[felnd] = -3.0e38                                                       # nodata elevations under valid angles (own and receivers')
    wg = (0.5 + rng.random((ny, nx), dtype=np.float32) * 2.0).astype(np.float32)
    wg[rng.random((ny, nx)) < 0.01] = -9999.0                                  # nodata weights: contaminate, still count with wt = 1
    return g, ang, fel, src, wg


def make(exe, name, ranks=1, check_ranks=0):
    g, ang, fel, src, wg = inputs(name)
    ny, nx = ang.shape
    dx, dy, geographic = float(g["dx"]), float(g["dy"]), bool(g["geographic"])
    gt = (-111.9, dx, 0.0, 41.9, 0.0, -dy) if geographic else (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)
    res = {"ang": ang, "fel": fel, "src": src, "wg": wg, "dxc": g["dxc"], "dyc": g["dyc"], "src_nodata": np.int16(SRC_NODATA)}
    agree = []
    with tempfile.TemporaryDirectory() as d:
        f = lambda s: os.path.join(d, s)  # noqa: E731
        T.write_raster(f("ang.tif"), ang, -3.402823466e38, geotransform=gt, geographic=geographic)
        T.write_raster(f("fel.tif"), fel, -3.0e38, geotransform=gt, geographic=geographic)
        T.write_raster(f("src.tif"), src, SRC_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("wg.tif"), wg, -9999.0, geotransform=gt, geographic=geographic)
        base = ["-ang", f("ang.tif"), "-fel", f("fel.tif"), "-slp", f("nonexistent_slp.tif"), "-src", f("src.tif")]
        for st in STATS:
            for kd in KINDS:
                for suffix, extra in (("", []), ("_nc", ["-nc"]), ("_wg", ["-wg", f("wg.tif")])):
                    out = f(f"dd_{st}_{kd}{suffix}.tif")
                    O.run_ref(exe, base + extra + ["-dd", out, "-m", st, kd], ranks)
                    res[f"dd_{st}_{kd}{suffix}"], _ = T.read_raster(out)
                    if check_ranks and suffix == "":
                        out3 = f(f"dd3_{st}_{kd}.tif")
                        O.run_ref(exe, base + ["-dd", out3, "-m", kd, st], check_ranks)   # (the two -m tokens in the other order)
                        a3, _ = T.read_raster(out3)
                        agree.append((st, kd, bool(np.array_equal(a3.view(np.uint32), res[f"dd_{st}_{kd}"].view(np.uint32)))))
    np.savez_compressed(os.path.join(OUT, f"distdown_{name}.npz"), **res)
    v = res["dd_ave_v"]
    print(name, ang.shape, "stream cells", int((src >= 1).sum()), "HAND max", float(v[v > -1e30].max()), "nodata", int((v < -1e30).sum()))
    if agree:
        print(f"  {check_ranks} ranks vs 1 rank:", "; ".join(f"{s} {k}: {'same' if a else 'DIFFERENT'}" for s, k, a in agree))


if __name__ == "__main__":
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_tool(tmp)
        for c in CASES:
            make(exe, c, check_ranks=3 if c == "holes" else 0)
