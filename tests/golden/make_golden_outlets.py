"""Golden vectors for MoveOutletsToStrm and ConnectDown (src/MoveOutletsToStrm.cpp, src/ConnectDown.cpp): runs the REAL reference tools on one
rank.  Build container only, after build() has left the reference's common objects in oracle/_ref/obj:

    python tests/golden/make_golden_outlets.py

Both tools are compiled into a temporary directory with the flags of oracle/Makefile's REFFLAGS; MoveOutletsToStrm.cpp and ConnectDown.cpp get
`-include tests/outlets/ogr_record_stub.h`, which records every feature they create as a line of text (see that header).  Nothing is written under
oracle/.  outlets_<case>.npz holds, for the five committed cases with the inputs of tests/outlets_model.inputs():
  * ox, oy, ids: the outlets' coordinates and ids (tests/outlets_model.OUTLET_KINDS says which is which);
  * move_md<m>: the record of moveoutletstostrm -md m as uint8, for m in MAXDISTS;
  * connect_o_d<d>, connect_od_d<d>: the records of connectdown -d d, for d in MOVEDISTS.
outlets_small.npz holds the same per hand-built raster of tests/outlets_model.small_rasters() under `<name>_<key>` (names in `names`), with the
outlets of small_outlets().  A raster on which ConnectDown finds no watershed has `<name>_nopoints` = 1 and no ConnectDown record: the reference
prints "No points found" and then runs on past MPI_Finalize, so how it ends is not its answer.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import outlets_model as M  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
MPI_ROOT = "/opt/conda"
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
STUB = os.path.join(ROOT, "tests", "outlets", "ogr_record_stub.h")


def build_tools(d):
    inc = ["-Igdal_shim", f"-I{os.path.join(ROOT, 'oracle', '_ref', 'mpiinc')}", f"-I{REF_SRC}"]
    flags = ["-std=c++17", "-O3", "-w"]   # oracle/Makefile REFFLAGS
    common = [os.path.join(OBJ, f + ".o") for f in ("commonLib", "tiffIO", "ReadOutlets", "shim", "geotiff", "outlets")]
    exes = {}
    for tool, main in (("MoveOutletsToStrm", "MoveOutletsToStrmmn"), ("ConnectDown", "ConnectDownmn")):
        objs = []
        for s in (tool, main):
            o = os.path.join(d, s + ".o")
            extra = ["-include", STUB] if s == tool else []
            subprocess.run(["g++"] + flags + inc + extra + ["-c", os.path.join(REF_SRC, s + ".cpp"), "-o", o], check=True, cwd=os.path.join(ROOT, "oracle"))
            objs.append(o)
        exes[tool] = os.path.join(d, tool.lower())
        subprocess.run(["g++"] + objs + common + [f"{MPI_ROOT}/lib/libmpi.so", f"-Wl,-rpath,/usr/lib/x86_64-linux-gnu:{MPI_ROOT}/lib", "-Wl,--allow-shlib-undefined",
                                                   "-lz", "-o", exes[tool]], check=True)
    return exes


def run_tool(exe, args, timeout=120):
    env = dict(os.environ)
    env["PATH"] = "/opt/conda/bin:" + env.get("PATH", "")
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=env)


def rec(path):
    return np.frombuffer(open(path + ".rec", "rb").read(), np.uint8)


def run_both(exes, p, src, w, ad8, gt, geographic, outlets):
    """The records of both tools for every -md / -d; (dict, whether ConnectDown found a watershed)."""
    cols, rows, ids = outlets
    ox, oy = M.cell_centre(gt, cols, rows)
    res = {"ox": ox, "oy": oy, "ids": np.asarray(ids, np.int32)}
    with tempfile.TemporaryDirectory() as d:
        f = lambda s: os.path.join(d, s)  # noqa: E731
        T.write_raster(f("p.tif"), p, M.P_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("src.tif"), src.astype(np.int16), M.SRC_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("w.tif"), w, M.W_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("ad8.tif"), ad8, M.AD8_NODATA, geotransform=gt, geographic=geographic)
        with open(f("outlets.txt"), "w") as fo:
            for x, y, i in zip(ox, oy, ids):
                fo.write(f"{float(x)!r} {float(y)!r} {int(i)}\n")
        for md in M.MAXDISTS:
            r = run_tool(exes["MoveOutletsToStrm"], ["-p", f("p.tif"), "-src", f("src.tif"), "-o", f("outlets.txt"), "-om", f(f"moved{md}.shp"), "-md", md])
            assert r.returncode == 0, (r.returncode, r.stdout[-800:], r.stderr[-800:])
            res[f"move_md{md}"] = rec(f(f"moved{md}.shp"))
        found = bool(np.any(w != M.W_NODATA))
        for dd in M.MOVEDISTS:
            r = run_tool(exes["ConnectDown"], ["-p", f("p.tif"), "-w", f("w.tif"), "-ad8", f("ad8.tif"), "-o", f(f"o{dd}.shp"), "-od", f(f"od{dd}.shp"), "-d", dd])
            if not found:
                assert "No points found" in r.stdout, r.stdout[-800:]
                print("    no watershed: the reference says so, then ends with", r.returncode)
                continue
            assert r.returncode == 0, (r.returncode, r.stdout[-800:], r.stderr[-800:])
            res[f"connect_o_d{dd}"], res[f"connect_od_d{dd}"] = rec(f(f"o{dd}.shp")), rec(f(f"od{dd}.shp"))
    return res, found


def main():
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exes = build_tools(tmp)
        for name in M.CASES:
            p, src, w, ad8, gt, geographic = M.inputs(name)
            outlets = M.outlet_points(p, src)
            far = M.check_outlet_points(p, src, outlets[0], outlets[1])
            ties = M.tied_watersheds(w, ad8)
            assert ties, name
            res, _ = run_both(exes, p, src, w, ad8, gt, geographic, outlets)
            np.savez_compressed(os.path.join(OUT, f"outlets_{name}.npz"), **res)
            print(name, p.shape, "farthest outlet", far, "steps; watersheds with a tied maximum", len(ties), "bytes", os.path.getsize(os.path.join(OUT, f"outlets_{name}.npz")))
        small, names = {}, []
        for name, (p, w, ad8) in M.small_rasters().items():
            print(" ", name)
            res, found = run_both(exes, p, M.small_src(w, ad8), w, ad8, M.SMALL_GT, False, M.small_outlets(p))
            names.append(name)
            small.update({f"{name}_{k}": v for k, v in res.items()})
            small[f"{name}_nopoints"] = np.array(0 if found else 1)
        small["names"] = np.array(names)
        np.savez_compressed(os.path.join(OUT, "outlets_small.npz"), **small)
        print("hand-built:", names)


if __name__ == "__main__":
    main()
