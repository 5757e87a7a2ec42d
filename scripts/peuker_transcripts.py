"""Transcripts of bin/peukerdouglas, in the form of scripts/dropan_transcripts.py (the run_one / differences / normalisation of scripts/tool_transcripts.py
are used): exit status, stdout and stderr with times blanked, SHA-256 of the stream-source raster, on the `plain` golden's fel with --gpus 1 and --gpus 2,
the default weights and a -par, and the error runs that end before the compute step and need no GPU (an input file that is missing, one that is no TIFF).

    python scripts/peuker_transcripts.py --record tests/golden/tool_transcripts_peuker.json     (on a GPU machine)
    python scripts/peuker_transcripts.py --check tests/golden/tool_transcripts_peuker.json [--kind err|gpu]
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
    import taudem_amd as T

    g = np.load(os.path.join(ROOT, "tests", "golden", "case_plain.npz"))
    os.makedirs(d, exist_ok=True)
    dx, dy, ny = float(g["dx"]), float(g["dy"]), g["fel"].shape[0]
    T.write_raster(os.path.join(d, "fel.tif"), g["fel"], float(T.FEL_NODATA), geotransform=(1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy))
    open(os.path.join(d, "text.tif"), "w").write("not a raster\n")


def runs(kind):
    if kind == "err":
        # (the usage runs - a -par cut short, an unknown flag - print the program's own path and are not recorded: tests/test_gpu_peuker.py looks at them)
        return [("err/peukerdouglas/missing_fel", ["-fel", "@nope", "-ss", ">ss.tif"], 1), ("err/peukerdouglas/not_a_tiff", ["-fel", "@text", "-ss", ">ss.tif"], 1)]
    return [(f"gpu{gpus}/plain/peukerdouglas/{tag}", ["-fel", "@fel", "-ss", ">ss.tif", *par], gpus) for gpus in (1, 2)
            for tag, par in (("default", []), ("par", ["-par", "0.5", "0.125", "0"]))]


def collect(kind):
    tt = _tt()
    got = {}
    with tempfile.TemporaryDirectory(prefix="tdx_peuker_transcripts_") as d:
        d = os.path.realpath(d)
        indir = os.path.join(d, "plain")
        write_inputs(indir)
        for rid, args, gpus in runs(kind):
            t = tt.run_one(d, rid.replace("/", "_"), indir, "peukerdouglas", args, gpus)
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
