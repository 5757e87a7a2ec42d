"""Transcripts of bin/moveoutletstostrm and bin/connectdown, in the form of scripts/streamnet_transcripts.py (the run_one / differences / normalisation of
scripts/tool_transcripts.py are used): exit status, stdout and stderr with times blanked, SHA-256 of the written layer files, on the `holes` inputs of
the outlet goldens - the error runs that end before the compute step and need no GPU (a raster that is missing, a raster of another size, an output
extension no layer writer exists for), and the runs on one GPU and on three rank threads.

    python scripts/outlets_transcripts.py --record tests/golden/tool_transcripts_outlets.json [--kind err|gpu]    (gpu: on a GPU machine)
    python scripts/outlets_transcripts.py --check tests/golden/tool_transcripts_outlets.json [--kind err|gpu]
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MOVED = [">moved.shp", ">moved.shx", ">moved.dbf"]


def _tt():
    spec = importlib.util.spec_from_file_location("tool_transcripts", os.path.join(ROOT, "scripts", "tool_transcripts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def write_inputs(d):
    import outlets_model as M
    import taudem_amd as T

    p, src, w, ad8, gt, _ = M.inputs("holes")
    g = M.load_golden("holes")
    os.makedirs(d, exist_ok=True)
    T.write_raster(os.path.join(d, "p.tif"), p, M.P_NODATA, geotransform=gt)
    T.write_raster(os.path.join(d, "src.tif"), src.astype(np.int16), M.SRC_NODATA, geotransform=gt)
    T.write_raster(os.path.join(d, "w.tif"), w, M.W_NODATA, geotransform=gt)
    T.write_raster(os.path.join(d, "ad8.tif"), ad8, M.AD8_NODATA, geotransform=gt)
    T.write_raster(os.path.join(d, "psmall.tif"), np.ascontiguousarray(p[:-3]), M.P_NODATA, geotransform=gt)
    T.write_raster(os.path.join(d, "ad8small.tif"), np.ascontiguousarray(ad8[:, :-2]), M.AD8_NODATA, geotransform=gt)
    with open(os.path.join(d, "outlets.txt"), "w") as fo:
        for x, y, k in zip(g["ox"], g["oy"], g["ids"]):
            fo.write(f"{float(x)!r} {float(y)!r} {int(k)}\n")


def _outs(*names):
    return [">" + n for n in names]


def runs(kind):
    move = ["-p", "@p", "-src", "@src", "-o", "@@outlets.txt"]
    conn = ["-p", "@p", "-w", "@w", "-ad8", "@ad8"]
    if kind == "err":
        return [("err/moveoutletstostrm/missing_src", "moveoutletstostrm", ["-p", "@p", "-src", "@nope", "-o", "@@outlets.txt", "-om", ">moved.shp", "-md", "50"], _outs("moved.shx", "moved.dbf"), 1),
                ("err/moveoutletstostrm/p_of_another_size", "moveoutletstostrm", ["-p", "@psmall", "-src", "@src", "-o", "@@outlets.txt", "-om", ">moved.shp", "-md", "50"], _outs("moved.shx", "moved.dbf"), 1),
                ("err/moveoutletstostrm/missing_outlets", "moveoutletstostrm", ["-p", "@p", "-src", "@src", "-o", "@@nope.shp", "-om", ">moved.shp", "-md", "50"], _outs("moved.shx", "moved.dbf"), 1),
                ("err/moveoutletstostrm/kml_refused", "moveoutletstostrm", [*move, "-om", ">moved.kml", "-md", "50"], [], 1),
                ("err/connectdown/missing_w", "connectdown", ["-p", "@p", "-w", "@nope", "-ad8", "@ad8", "-o", ">o.shp", "-od", ">od.geojson"], _outs("o.shx", "o.dbf"), 1),
                ("err/connectdown/p_of_another_size", "connectdown", ["-p", "@psmall", "-w", "@w", "-ad8", "@ad8", "-o", ">o.shp", "-od", ">od.geojson"], _outs("o.shx", "o.dbf"), 1),
                ("err/connectdown/ad8_of_another_size", "connectdown", ["-p", "@p", "-w", "@w", "-ad8", "@ad8small", "-o", ">o.shp", "-od", ">od.geojson"], _outs("o.shx", "o.dbf"), 1),
                ("err/connectdown/sqlite_refused", "connectdown", [*conn, "-o", ">o.shp", "-od", ">od.sqlite", "-d", "3"], _outs("o.shx", "o.dbf"), 1)]
    out = []
    for gpus in (1, 3):
        out.append((f"gpu{gpus}/holes/moveoutletstostrm/md50", "moveoutletstostrm", [*move, "-om", ">moved.shp", "-md", "50"], _outs("moved.shx", "moved.dbf"), gpus))
        out.append((f"gpu{gpus}/holes/connectdown/d10", "connectdown", [*conn, "-o", ">o.shp", "-od", ">od.geojson", "-d", "10"], _outs("o.shx", "o.dbf"), gpus))
    return out


def collect(kind):
    tt = _tt()
    got = {}
    with tempfile.TemporaryDirectory(prefix="tdx_outlets_transcripts_") as d:
        d = os.path.realpath(d)
        indir = os.path.join(d, "holes")
        write_inputs(indir)
        for rid, tool, args, more, gpus in runs(kind):
            t = tt.run_one(d, rid.replace("/", "_"), indir, tool, args, gpus)
            out = os.path.join(d, "out", rid.replace("/", "_"))
            t["files"].update({n[1:]: tt._sha(os.path.join(out, n[1:])) for n in more})   # the files a .shp brings with it
            got[rid] = t
            if kind == "gpu" and t["status"] != 0:   # a GPU run that fails may have left the card in a bad state: nothing more is started on it
                print(f"{rid} ended with status {t['status']}: no further GPU run is started", file=sys.stderr)
                break
    return got


def load_fixture(path, kind):
    return _tt().load_fixture(path, kind)


def differences(expected, got):
    return _tt().differences(expected, got)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--record", metavar="JSON")
    ap.add_argument("--check", metavar="JSON")
    ap.add_argument("--kind", choices=["err", "gpu", "all"], default="all")
    a = ap.parse_args()
    kinds = ["err", "gpu"] if a.kind == "all" else [a.kind]
    got = {}
    for kind in kinds:
        got.update(collect(kind))
    if a.record:
        old = {}
        if os.path.exists(a.record):   # the runs of the other kind stay as they are
            with open(a.record) as f:
                old = {rid: t for rid, t in json.load(f).items() if all(rid.startswith("err/") != (kind == "err") for kind in kinds)}
        old.update(got)
        with open(a.record, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(rid)}: {json.dumps(old[rid], sort_keys=True)}" for rid in sorted(old)) + "\n}\n")
        print(f"recorded {len(got)} runs ({len(old)} in {a.record})")
    if a.check:
        expected = {}
        for kind in kinds:
            expected.update(load_fixture(a.check, kind))
        bad = differences(expected, got)
        print("\n".join(bad) if bad else f"{len(got)} transcripts reproduced")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
