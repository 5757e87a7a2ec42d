"""Golden vectors for DinfDistUp (src/DinfDistUp.cpp): runs the REAL reference tool on the D-infinity angles and pit-filled elevations
of the committed cases.  Build container only, after build() has left the reference's common objects in oracle/_ref/obj:

    python tests/golden/make_golden_distup.py

The reference tool is compiled into a temporary directory (the flags of oracle/Makefile's REFFLAGS, linked against oracle/_ref/obj);
nothing is written under oracle/.  distup_<case>.npz holds the inputs (ang with a few interior cells without an angle, fel with a few
nodata cells under valid angles, weights with a few negative and a few nodata cells, per-row cell sizes) and, for every -m combination, the reference's
raster with the default contamination check (du_<stat>_<type>), with -nc (..._nc) and with -wg (..._wg; for v only `ave`, since v
ignores the weights), plus -thresh 0.3 runs of ave h and max v (..._t); tests/distup_model.variants() lists them.  The weights are
multiples of 1/8 so that the weight raster compresses.  The files are named distup_*.npz, not case_*.npz: conftest.golden_cases() takes every case_*.npz as a
case.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distup_model as M  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
MPI_ROOT = "/opt/conda"
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
CASES = ("plain", "holes", "rect_dxdy", "geographic", "fourway_mask")


def build_tool(d):
    """Compiles the reference's DinfDistUp into directory d; returns the executable."""
    inc = ["-Igdal_shim", f"-I{os.path.join(ROOT, 'oracle', '_ref', 'mpiinc')}", f"-I{REF_SRC}"]
    flags = ["-std=c++17", "-O3", "-w"]   # oracle/Makefile REFFLAGS
    objs = []
    for s in ("DinfDistUp", "DinfDistUpmn"):
        o = os.path.join(d, s + ".o")
        subprocess.run(["g++"] + flags + inc + ["-c", os.path.join(REF_SRC, s + ".cpp"), "-o", o], check=True, cwd=os.path.join(ROOT, "oracle"))
        objs.append(o)
    common = [os.path.join(OBJ, f + ".o") for f in ("commonLib", "tiffIO", "ReadOutlets", "shim", "geotiff", "outlets")]
    exe = os.path.join(d, "dinfdistup")
    subprocess.run(["g++"] + objs + common + [f"{MPI_ROOT}/lib/libmpi.so", f"-Wl,-rpath,/usr/lib/x86_64-linux-gnu:{MPI_ROOT}/lib", "-Wl,--allow-shlib-undefined",
                                              "-lz", "-o", exe], check=True)
    return exe


def inputs(name):
    g = np.load(os.path.join(OUT, f"case_{name}.npz"))
    ang = g["ang"].copy()
    fel = g["fel"].copy()
    ny, nx = ang.shape
    rng = np.random.default_rng(900 + nx + ny)
    inner = np.zeros((ny, nx), bool)
    inner[2:-2, 2:-2] = True
    ang[inner & (rng.random((ny, nx)) < 0.002)] = -3.402823466e38        # interior cells without an angle: contaminate their neighbours
    felnd = (rng.random((ny, nx)) < 0.004) & (ang > -1e30)
    fel[felnd] = -3.0e38                                                 # nodata elevations under valid angles (v: no own-elevation test)
    wg = (0.5 + rng.integers(0, 17, (ny, nx)) / 8.0).astype(np.float32)   # 0.5 .. 2.5 in steps of 1/8
    neg = rng.random((ny, nx)) < 0.05
    wg[neg] = -wg[neg]                                                   # negative weights: negative h steps, where `max h` from 0 shows
    wg[rng.random((ny, nx)) < 0.01] = -9999.0                            # nodata weights: contaminate, still count with wt = 1
    return g, ang, fel, wg


def make(exe, name, check_ranks=0):
    g, ang, fel, wg = inputs(name)
    ny, nx = ang.shape
    dx, dy, geographic = float(g["dx"]), float(g["dy"]), bool(g["geographic"])
    gt = (-111.9, dx, 0.0, 41.9, 0.0, -dy) if geographic else (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)
    res = {"ang": ang, "fel": fel, "wg": wg, "dxc": g["dxc"], "dyc": g["dyc"]}
    agree = []
    with tempfile.TemporaryDirectory() as d:
        f = lambda s: os.path.join(d, s)  # noqa: E731
        T.write_raster(f("ang.tif"), ang, -3.402823466e38, geotransform=gt, geographic=geographic)
        T.write_raster(f("fel.tif"), fel, -3.0e38, geotransform=gt, geographic=geographic)
        T.write_raster(f("wg.tif"), wg, -9999.0, geotransform=gt, geographic=geographic)
        base = ["-ang", f("ang.tif"), "-fel", f("fel.tif"), "-slp", f("nonexistent_slp.tif")]
        extras = {"": [], "_nc": ["-nc"], "_wg": ["-wg", f("wg.tif")], "_t": ["-thresh", str(M.THRESH)]}
        for st, kd, suffix in M.variants():
            out = f(f"du_{st}_{kd}{suffix}.tif")
            O.run_ref(exe, base + extras[suffix] + ["-du", out, "-m", st, kd])
            res[f"du_{st}_{kd}{suffix}"], _ = T.read_raster(out)
            if check_ranks and suffix in ("", "_t"):
                out3 = f(f"du3_{st}_{kd}{suffix}.tif")
                O.run_ref(exe, base + extras[suffix] + ["-du", out3, "-m", kd, st], check_ranks)   # (the two -m tokens in the other order)
                a3, _ = T.read_raster(out3)
                agree.append((st, kd + suffix, bool(np.array_equal(a3.view(np.uint32), res[f"du_{st}_{kd}{suffix}"].view(np.uint32)))))
    np.savez_compressed(os.path.join(OUT, f"distup_{name}.npz"), **res)
    v = res["du_ave_h"]
    print(name, ang.shape, "ave h max", float(v[v > -1e30].max()), "nodata", int((v < -1e30).sum()), "nodata -nc", int((res["du_ave_h_nc"] < -1e30).sum()))
    if agree:
        print(f"  {check_ranks} ranks vs 1 rank:", "; ".join(f"{s} {k}: {'same' if a else 'DIFFERENT'}" for s, k, a in agree))
        assert all(a for _, _, a in agree), "the reference's multi-rank run differs from its 1-rank run on a projected case"


if __name__ == "__main__":
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_tool(tmp)
        for c in CASES:
            make(exe, c, check_ranks=3 if c in ("holes", "plain", "rect_dxdy") else 0)
