"""Golden vectors for StreamNet (src/streamnet.cpp): runs the REAL reference tool on one rank.  Build container only, after build() has left the
reference's common objects in oracle/_ref/obj:

    python tests/golden/make_golden_streamnet.py

The tool is compiled into a temporary directory with the flags of oracle/Makefile's REFFLAGS; streamnet.cpp alone gets
`-include tests/streamnet/ogr_write_stub.h`, which turns the OGR write calls of the -net layer into no-ops (no golden holds that layer).  Nothing is
written under oracle/.  streamnet_<case>.npz holds, for the five committed cases with src = ad8 >= THRESH[case] (a few cells raised to 2):
  * p (the case's, with one stream led off the west edge), src, the geotransform, the outlets (columns / rows / ids);
  * ord_<v>, w_<v>, tree_<v>, coord_<v> (the files' bytes as uint8) for v in plain (no outlets), outlets (-o), sw (-sw).
streamnet_small.npz holds the same for the hand-built rasters of tests/streamnet_model.py (names in `names`; v in plain, outlets, sw).  A
hand-built raster on which the reference does not exit with 0 within 120 s is left out and named on stdout.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import streamnet_model as M  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
MPI_ROOT = "/opt/conda"
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
STUB = os.path.join(ROOT, "tests", "streamnet", "ogr_write_stub.h")


def build_tool(d):
    inc = ["-Igdal_shim", f"-I{os.path.join(ROOT, 'oracle', '_ref', 'mpiinc')}", f"-I{REF_SRC}"]
    flags = ["-std=c++17", "-O3", "-w"]   # oracle/Makefile REFFLAGS
    objs = []
    for s in ("streamnet", "streamnetmn"):
        o = os.path.join(d, s + ".o")
        extra = ["-include", STUB] if s == "streamnet" else []
        subprocess.run(["g++"] + flags + inc + extra + ["-c", os.path.join(REF_SRC, s + ".cpp"), "-o", o], check=True, cwd=os.path.join(ROOT, "oracle"))
        objs.append(o)
    common = [os.path.join(OBJ, f + ".o") for f in ("commonLib", "tiffIO", "ReadOutlets", "shim", "geotiff", "outlets")]
    exe = os.path.join(d, "streamnet")
    subprocess.run(["g++"] + objs + common + [f"{MPI_ROOT}/lib/libmpi.so", f"-Wl,-rpath,/usr/lib/x86_64-linux-gnu:{MPI_ROOT}/lib", "-Wl,--allow-shlib-undefined",
                                              "-lz", "-o", exe], check=True)
    return exe


def run_variants(exe, p, src, fel, ad8, gt, geographic, outlets, timeout=120):
    """{key_<variant>: array} of the reference's four outputs for the three variants."""
    cols, rows, ids = outlets
    dx, dy = abs(gt[1]), abs(gt[5])
    res = {}
    with tempfile.TemporaryDirectory() as d:
        f = lambda s: os.path.join(d, s)  # noqa: E731
        T.write_raster(f("p.tif"), p, M.P_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("src.tif"), src, M.SRC_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("fel.tif"), fel, -3.0e38, geotransform=gt, geographic=geographic)
        T.write_raster(f("ad8.tif"), ad8, -1.0, geotransform=gt, geographic=geographic)
        with open(f("outlets.txt"), "w") as fo:
            for c, r, i in zip(cols, rows, ids):
                fo.write(f"{float(gt[0] + (c + 0.5) * dx)!r} {float(gt[3] - (r + 0.5) * dy)!r} {i}\n")
        for v in M.VARIANTS:
            args = ["-p", f("p.tif"), "-src", f("src.tif"), "-fel", f("fel.tif"), "-ad8", f("ad8.tif"), "-ord", f(v + "ord.tif"), "-w", f(v + "w.tif"),
                    "-tree", f(v + "tree.txt"), "-coord", f(v + "coord.txt"), "-net", f(v + "net.shp")]
            args += {"plain": [], "outlets": ["-o", f("outlets.txt")], "sw": ["-sw"]}[v]
            O.run_ref(exe, args, timeout=timeout)
            res["ord_" + v], _ = T.read_raster(f(v + "ord.tif"), np.int16)
            res["w_" + v], _ = T.read_raster(f(v + "w.tif"), np.int32)
            res["tree_" + v] = np.frombuffer(open(f(v + "tree.txt"), "rb").read(), np.uint8)
            res["coord_" + v] = np.frombuffer(open(f(v + "coord.txt"), "rb").read(), np.uint8)
    return res


def tree_rows(b):
    t = bytes(b).decode()
    return np.array([[int(v) for v in line.split()] for line in t.splitlines()], np.int64).reshape(-1, 9)


def main():
    O.build()
    seen = {"k3": False, "edge": False, "two": False}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_tool(tmp)
        for name in M.CASES:
            g, p, src = M.inputs(name)
            ny, nx = p.shape
            geographic = bool(g["geographic"])
            gt = M.geotransform(nx, ny, float(g["dx"]), float(g["dy"]), geographic)
            outlets = M.outlets_for(p, src)
            res = run_variants(exe, p, src, g["fel"], g["ad8"], gt, geographic, outlets)
            res.update({"p": p, "src": src, "gt": np.array(gt), "cols": outlets[0], "rows": outlets[1], "ids": outlets[2]})
            np.savez_compressed(os.path.join(OUT, f"streamnet_{name}.npz"), **res)
            # what the inputs must exercise
            stream, recv, nin = M.stream_graph(p, src)
            tree = tree_rows(res["tree_plain"])
            assert len(tree) >= 20, (name, len(tree))
            seen["k3"] |= bool(np.any(nin[stream.ravel()] >= 3))
            seen["edge"] |= bool(np.any(stream.ravel() & (recv < 0) & (p.ravel() > 0)))
            seen["two"] |= bool(np.any(src == 2))
            cols, rows, _ = outlets
            oc = rows[:6].astype(np.int64) * nx + cols[:6]
            assert nin[oc[0]] >= 2 and nin[oc[1]] == 1 and nin[oc[2]] == 0 and stream.flat[oc[2]] and not stream.flat[oc[3]] and oc[4] == oc[5], name
            assert not (0 <= cols[6] < nx), name
            print(name, p.shape, "stream cells", int(stream.sum()), "links", len(tree), "with outlets", len(tree_rows(res["tree_outlets"])), "bytes",
                  os.path.getsize(os.path.join(OUT, f"streamnet_{name}.npz")))
        assert all(seen.values()), seen
        small, names, left_out = {}, [], []
        for name, (p, src) in M.small_rasters().items():
            fel, ad8 = M.small_fields(p)
            try:
                res = run_variants(exe, p, src, fel, ad8, M.SMALL_GT, False, M.SMALL_OUTLETS)
            except (RuntimeError, subprocess.TimeoutExpired) as e:
                left_out.append(name)
                print("left out:", name, str(e)[:200])
                continue
            names.append(name)
            small.update({f"{name}_{k}": v for k, v in res.items()})
        assert len(left_out) <= 2, left_out
        small["names"] = np.array(names)
        np.savez_compressed(os.path.join(OUT, "streamnet_small.npz"), **small)
        print("hand-built:", names, "left out:", left_out)


if __name__ == "__main__":
    main()
