"""Golden records of the stream network line layer and of CatchOutlets: runs the REAL reference tools on one rank.  Build container only, after build() has
left the reference's common objects in oracle/_ref/obj:

    python tests/golden/make_golden_netlayer.py

streamnet.cpp is compiled unmodified with `-include tests/streamnet/ogr_record_lines_stub.h`, which records every line feature the tool creates for its
-net layer; CatchOutlets.cpp with `-include tests/netlayer/ogr_replay_lines_stub.h`, which serves exactly that record back through the OGR read calls
the file uses and records the point features it creates.  Both go into a temporary directory; nothing is written under oracle/.

netlayer_<case>.npz (the five streamnet cases, on the inputs of streamnet_<case>.npz) and netlayer_small.npz (the hand-built rasters of
tests/streamnet_model.py that streamnet_small.npz holds, keys prefixed "<name>_") hold, as the bytes of the text, for v in plain, outlets:
    net_<v>            the line record: "<vertices> <x0> <y0> ... <field>=<value> ..." per link, %.17g
    exact_<v>          whether tests/netlayer_model.net_rows on the rows of the -tree / -coord TEXT of streamnet_<case>.npz gives that record bit for bit
                       (the text holds six decimals of float values: it does where every float of the links survives that)
    co_params_<v>      the (mindist, minarea, gwstartno) runs of netlayer_model.grid on the record
    co_<v>_<k>         the point record of CatchOutlets' run k on the record: "<x> <y> <field>=<value> ..." (the hand-built rasters: runs 0 and 3)
    co_plain_pzero     the run (0, 0, 1) on a flow direction raster whose cell under the first outlet link's down end (pzero_cell: column, row) is 0
(a network without a link has net_<v> and exact_<v> only)
The script ASSERTS: the tool with the recording stub writes the -tree and -coord bytes the committed streamnet fixtures hold; every CatchOutlets record
equals netlayer_model.catch_outlets on the line record; at least one PROJECTED case has exact_plain; and, over all
records: a link skipped by mindist alone, a subtree cut by minarea, an outlet link whose down end has a p outside 1..8, a down end whose step
would leave the raster, a first Id other than 1.  No file is larger than the largest outlets_*.npz.  (It also counts the links of a single point: the
reference's -coord rows hold the cell of a one-cell link twice, so none of these rasters has one; the one-vertex line is held by
tests/test_netlayer_rows.py on rows of its own.)
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import netlayer_model as N  # noqa: E402
import streamnet_model as M  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
MPI_ROOT = "/opt/conda"
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
STUBS = {"streamnet": os.path.join(ROOT, "tests", "streamnet", "ogr_record_lines_stub.h"), "CatchOutlets": os.path.join(ROOT, "tests", "netlayer", "ogr_replay_lines_stub.h")}


def build_tool(d, name, sources):
    inc = ["-Igdal_shim", f"-I{os.path.join(ROOT, 'oracle', '_ref', 'mpiinc')}", f"-I{REF_SRC}"]
    flags = ["-std=c++17", "-O3", "-w"]   # oracle/Makefile REFFLAGS
    objs = []
    for s in sources:
        o = os.path.join(d, s + ".o")
        extra = ["-include", STUBS[s]] if s in STUBS else []
        subprocess.run(["g++"] + flags + inc + extra + ["-c", os.path.join(REF_SRC, s + ".cpp"), "-o", o], check=True, cwd=os.path.join(ROOT, "oracle"))
        objs.append(o)
    common = [os.path.join(OBJ, f + ".o") for f in ("commonLib", "tiffIO", "ReadOutlets", "shim", "geotiff", "outlets")]
    exe = os.path.join(d, name)
    subprocess.run(["g++"] + objs + common + [f"{MPI_ROOT}/lib/libmpi.so", f"-Wl,-rpath,/usr/lib/x86_64-linux-gnu:{MPI_ROOT}/lib", "-Wl,--allow-shlib-undefined",
                                              "-lz", "-o", exe], check=True)
    return exe


def as_bytes(text):
    return np.frombuffer(text.encode(), np.uint8)


def run_case(exes, p, src, fel, ad8, gt, geographic, outlets, committed, prefix, seen, keep=(0, 1, 2, 3)):
    """the records of one raster; committed: the streamnet fixture that holds its -tree / -coord bytes under prefix + "tree_<v>" """
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
        for v in N.VARIANTS:
            args = ["-p", f("p.tif"), "-src", f("src.tif"), "-fel", f("fel.tif"), "-ad8", f("ad8.tif"), "-ord", f(v + "ord.tif"), "-w", f(v + "w.tif"),
                    "-tree", f(v + "tree.txt"), "-coord", f(v + "coord.txt"), "-net", f(v + "net.shp")]
            args += {"plain": [], "outlets": ["-o", f("outlets.txt")]}[v]
            O.run_ref(exes["streamnet"], args, timeout=120)
            tree_b, coord_b = open(f(v + "tree.txt"), "rb").read(), open(f(v + "coord.txt"), "rb").read()
            assert tree_b == bytes(committed[f"{prefix}tree_{v}"]) and coord_b == bytes(committed[f"{prefix}coord_{v}"]), f"{prefix}{v}: -tree / -coord differ from the fixture"
            net = open(f(v + "net.shp.rec")).read()
            fields, lines = N.parse_lines(net)
            tree, coord = N.rows_of_text(tree_b, coord_b)
            assert len(lines) == len(tree) and all(len(ln) == t[2] - t[1] + 1 for ln, t in zip(lines, tree)), f"{prefix}{v}: vertex counts"
            seen["one_vertex"] += sum(len(ln) == 1 for ln in lines)
            exact = N.same_layer(N.net_rows(tree, coord, geographic), (fields, lines)) if len(tree) else True
            res[f"{prefix}net_{v}"], res[f"{prefix}exact_{v}"] = as_bytes(net), np.bool_(exact)
            if not lines:   # a network without a link: the record holds no field name the replay could serve, and CatchOutlets has nothing to do
                continue
            runs = N.grid(fields)
            res[f"{prefix}co_params_{v}"] = np.array(runs, np.float64)
            todo = [(str(k), run, p) for k, run in enumerate(runs) if k in keep]
            outlet_links = [i for i in range(len(lines)) if fields["DSLINKNO"][i] < 0]
            if v == "plain" and outlet_links:
                x, y = lines[outlet_links[0]][0]
                cx, cy = int((x - gt[0]) / dx), int((gt[3] - y) / dy)
                pz = p.copy()
                pz[cy, cx] = 0
                T.write_raster(f("pzero.tif"), pz, M.P_NODATA, geotransform=gt, geographic=geographic)
                res[f"{prefix}pzero_cell"] = np.array([cx, cy], np.int64)
                todo.append(("pzero", (0.0, 0.0, 1), pz))
            for k, (md, ma, gw), pk in todo:
                out = f(f"{v}co{k}.shp")
                O.run_ref(exes["catchoutlets"], ["-p", f("pzero.tif" if k == "pzero" else "p.tif"), "-net", f(v + "net.shp.rec"), "-o", out, "-mindist", repr(md), "-minarea", repr(ma),
                                                 "-gwstartno", str(gw)], timeout=120)
                rec = open(out + ".rec").read()
                want = N.catch_outlets(fields, lines, pk, gt, md, ma, gw, seen) if len(lines) else []
                assert N.parse_points(rec) == want, f"{prefix}{v} run {k}: the model differs from the tool"
                seen["ids"] |= {w[2]["Id"] for w in want[:1]}
                res[f"{prefix}co_{v}_{k}"] = as_bytes(rec)
    return res


def main():
    O.build()
    seen = {"one_vertex": 0, "ids": set()}
    limit = max(os.path.getsize(f) for f in glob.glob(os.path.join(OUT, "outlets_*.npz")))
    with tempfile.TemporaryDirectory() as tmp:
        exes = {"streamnet": build_tool(tmp, "streamnet", ("streamnet", "streamnetmn")), "catchoutlets": build_tool(tmp, "catchoutlets", ("CatchOutlets", "CatchOutletsmn"))}
        exact_projected = []
        for name in M.CASES:
            g, p, src = M.inputs(name)
            ny, nx = p.shape
            geographic = bool(g["geographic"])
            gt = M.geotransform(nx, ny, float(g["dx"]), float(g["dy"]), geographic)
            committed = M.load_golden(name)
            res = run_case(exes, p, src, g["fel"], g["ad8"], gt, geographic, M.outlets_for(p, src), committed, "", seen)
            path = os.path.join(OUT, f"netlayer_{name}.npz")
            np.savez_compressed(path, **res)
            if not geographic and bool(res["exact_plain"]):
                exact_projected.append(name)
            assert os.path.getsize(path) <= limit, (name, os.path.getsize(path), limit)
            print(name, p.shape, "links", len(N.parse_lines(N.text(res["net_plain"]))[1]), "exact", bool(res["exact_plain"]), bool(res["exact_outlets"]), "bytes", os.path.getsize(path))
        assert exact_projected, "no projected case whose -tree / -coord text reproduces the record"
        committed = M.load_golden("small")
        small = {}
        for name, (p, src) in M.small_rasters().items():
            if name not in [str(n) for n in committed["names"]]:
                continue
            fel, ad8 = M.small_fields(p)
            small.update(run_case(exes, p, src, fel, ad8, M.SMALL_GT, False, M.SMALL_OUTLETS, committed, name + "_", seen, keep=(0, 3)))
        small["names"] = committed["names"]
        path = os.path.join(OUT, "netlayer_small.npz")
        np.savez_compressed(path, **small)
        assert os.path.getsize(path) <= limit, (os.path.getsize(path), limit)
        print("hand-built:", [str(n) for n in small["names"]], "bytes", os.path.getsize(path))
    print("projected cases whose text is exact:", exact_projected, "seen:", {k: (sorted(v) if isinstance(v, set) else v) for k, v in seen.items()})
    assert seen["mindist"] and seen["minarea"] and seen["bad_p"] and seen["stays"] and seen["ids"] - {1}, seen


if __name__ == "__main__":
    main()
