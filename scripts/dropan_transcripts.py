"""Transcripts of bin/dropanalysis, in the form of scripts/tool_transcripts.py (whose run_one / differences / normalisation are used): exit status, stdout
and stderr with times blanked, SHA-256 of the table, on the `plain` golden with --gpus 1 and --gpus 2 and both step types, and the error runs that end
before the compute step and need no GPU (one threshold, an outlet file that is missing, an outlet on a cell without a direction, a direction raster of
another size).

    python scripts/dropan_transcripts.py --record tests/golden/tool_transcripts_dropan.json     (on a GPU machine)
    python scripts/dropan_transcripts.py --check tests/golden/tool_transcripts_dropan.json [--kind err|gpu]
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


def _tt():
    spec = importlib.util.spec_from_file_location("tool_transcripts", os.path.join(ROOT, "scripts", "tool_transcripts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def write_inputs(d):
    import dropan_model as M
    import taudem_amd as T

    g = M.load_golden("plain")
    os.makedirs(d, exist_ok=True)
    dx, dy, ny = float(g["dx"]), float(g["dy"]), g["p"].shape[0]
    gt = (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)
    T.write_raster(os.path.join(d, "p.tif"), g["p"], M.P_NODATA, geotransform=gt)
    T.write_raster(os.path.join(d, "small.tif"), g["p"][:-3], M.P_NODATA, geotransform=gt)
    T.write_raster(os.path.join(d, "fel.tif"), g["fel"], float(T.FEL_NODATA), geotransform=gt)
    T.write_raster(os.path.join(d, "ad8.tif"), g["ad8"], -1.0, geotransform=gt)
    line = lambda c, r, i: f"{float(gt[0] + (c + 0.5) * dx)!r} {float(gt[3] - (r + 0.5) * dy)!r} {i}\n"  # noqa: E731
    good = "".join(line(c, r, i + 1) for i, (c, r) in enumerate(zip(g["cols"], g["rows"])))
    ys, xs = np.nonzero(g["p"] == M.P_NODATA)
    open(os.path.join(d, "outlets.txt"), "w").write(good)
    open(os.path.join(d, "bad.txt"), "w").write(good + line(xs[0], ys[0], 99))
    return [str(float(v)) if i < 2 else str(int(v)) for i, v in enumerate(g["par"])]


def base(par, st, **swap):
    a = {"ad8": "@ad8", "p": "@p", "fel": "@fel", "ssa": "@ad8", "o": "@@outlets.txt"}
    a.update(swap)
    return ["-ad8", a["ad8"], "-p", a["p"], "-fel", a["fel"], "-ssa", a["ssa"], "-o", a["o"], "-drp", ">drp.txt", "-par", *par, str(st)]


def runs(kind, par):
    if kind == "err":
        # (the usage runs - no -o, a -par cut short - print the program's own path and are not recorded: tests/test_gpu_dropan.py looks at them)
        return [("err/dropanalysis/one_threshold", base([par[0], par[1], "1"], 0), 1), ("err/dropanalysis/missing_outlets", base(par, 0, o="@@nope.txt"), 1),
                ("err/dropanalysis/outlet_without_direction", base(par, 0, o="@@bad.txt"), 1), ("err/dropanalysis/small_p", base(par, 0, p="@small"), 1)]
    return [(f"gpu{gpus}/plain/dropanalysis/steptype{st}", base(par, st), gpus) for gpus in (1, 2) for st in (0, 1)]


def collect(kind):
    tt = _tt()
    got = {}
    with tempfile.TemporaryDirectory(prefix="tdx_dropan_transcripts_") as d:
        d = os.path.realpath(d)
        indir = os.path.join(d, "plain")
        par = write_inputs(indir)
        for rid, args, gpus in runs(kind, par):
            t = tt.run_one(d, rid.replace("/", "_"), indir, "dropanalysis", args, gpus)
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
        with open(a.record, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(rid)}: {json.dumps(got[rid], sort_keys=True)}" for rid in sorted(got)) + "\n}\n")
        print(f"recorded {len(got)} runs in {a.record}")
    if a.check:
        expected = {}
        for kind in kinds:
            expected.update(load_fixture(a.check, kind))
        bad = differences(expected, got)
        print("\n".join(bad) if bad else f"{len(got)} transcripts reproduced")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
