"""Transcripts of bin/streamnet, in the form of scripts/peuker_transcripts.py (the run_one / differences / normalisation of scripts/tool_transcripts.py
are used): exit status, stdout and stderr with times blanked, SHA-256 of the order and watershed rasters and of the tree and coord files, on the `holes`
inputs of the StreamNet goldens without outlets, with outlets, with -sw and with -v on one GPU, with outlets on two and with -sw on five rank threads, and the error runs that end before the compute step and need no
GPU (a src file that is missing, a p raster of another size, the -net layer that is not written).

    python scripts/streamnet_transcripts.py --record tests/golden/tool_transcripts_streamnet.json [--kind err|gpu]    (gpu: on a GPU machine)
    python scripts/streamnet_transcripts.py --check tests/golden/tool_transcripts_streamnet.json [--kind err|gpu]
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
OUTPUTS = ["-ord", ">ord.tif", "-w", ">w.tif", "-tree", ">tree.txt", "-coord", ">coord.txt"]


def _tt():
    spec = importlib.util.spec_from_file_location("tool_transcripts", os.path.join(ROOT, "scripts", "tool_transcripts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def write_inputs(d):
    import streamnet_model as M
    import taudem_amd as T

    g, c = M.load_golden("holes"), M.case_fields("holes")
    os.makedirs(d, exist_ok=True)
    gt = tuple(g["gt"])
    T.write_raster(os.path.join(d, "p.tif"), g["p"], M.P_NODATA, geotransform=gt)
    T.write_raster(os.path.join(d, "src.tif"), g["src"].astype(np.int16), M.SRC_NODATA, geotransform=gt)
    T.write_raster(os.path.join(d, "fel.tif"), c["fel"], -3.0e38, geotransform=gt)
    T.write_raster(os.path.join(d, "ad8.tif"), c["ad8"], -1.0, geotransform=gt)
    T.write_raster(os.path.join(d, "psmall.tif"), np.ascontiguousarray(g["p"][:-3]), M.P_NODATA, geotransform=gt)
    with open(os.path.join(d, "outlets.txt"), "w") as fo:
        for col, row, k in zip(g["cols"], g["rows"], g["ids"]):
            fo.write(f"{float(gt[0] + (col + 0.5) * abs(gt[1]))!r} {float(gt[3] - (row + 0.5) * abs(gt[5]))!r} {k}\n")


def runs(kind):
    inputs = ["-p", "@p", "-src", "@src", "-fel", "@fel", "-ad8", "@ad8"]
    if kind == "err":
        return [("err/streamnet/missing_src", ["-p", "@p", "-src", "@nope", "-fel", "@fel", "-ad8", "@ad8", *OUTPUTS], 1),
                ("err/streamnet/p_of_another_size", ["-p", "@psmall", "-src", "@src", "-fel", "@fel", "-ad8", "@ad8", *OUTPUTS], 1),
                ("err/streamnet/net_refused", [*inputs, *OUTPUTS, "-net", ">net.shp"], 1)]
    return [(f"gpu{gpus}/holes/streamnet/{tag}", [*inputs, *OUTPUTS, *extra], gpus)
            for gpus, tag, extra in ((1, "plain", []), (1, "outlets", ["-o", "@@outlets.txt"]), (1, "sw", ["-sw"]), (1, "verbose", ["-v", "-o", "@@outlets.txt"]),
                                     (2, "outlets", ["-o", "@@outlets.txt"]), (5, "sw", ["-sw"]))]

def collect(kind):
    tt = _tt()
    got = {}
    with tempfile.TemporaryDirectory(prefix="tdx_streamnet_transcripts_") as d:
        d = os.path.realpath(d)
        indir = os.path.join(d, "holes")
        write_inputs(indir)
        for rid, args, gpus in runs(kind):
            t = tt.run_one(d, rid.replace("/", "_"), indir, "streamnet", args, gpus)
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
