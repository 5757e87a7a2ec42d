"""Transcripts of bin/editraster, in the form of scripts/outlets_transcripts.py (the run_one / differences / normalisation of scripts/tool_transcripts.py are
used): exit status, stdout and stderr with times blanked, SHA-256 of the written raster, on the `wide` raster (67 x 5) of tests/editraster_model.py - the
runs that end before the compute step and need no GPU (a raster or a change file that is missing, a value no int16 holds), and the runs on one GPU and
on three rank threads.  (The usage text names the program as it was called: tests/test_editraster_host.py looks at it.)

    python scripts/editraster_transcripts.py --record tests/golden/tool_transcripts_editraster.json [--kind err|gpu]    (gpu: on a GPU machine)
    python scripts/editraster_transcripts.py --check tests/golden/tool_transcripts_editraster.json [--kind err|gpu]
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _tt():
    spec = importlib.util.spec_from_file_location("tool_transcripts", os.path.join(ROOT, "scripts", "tool_transcripts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def write_inputs(d):
    import editraster_model as M
    import taudem_amd as T

    a, nodata, files = M.cases()["wide"]
    gt = M.geotransform(a.shape[0])
    os.makedirs(d, exist_ok=True)
    T.write_raster(os.path.join(d, "in.tif"), a, int(nodata), geotransform=gt)
    for name, text in files.items():
        with open(os.path.join(d, name + ".txt"), "w") as f:
            f.write(text)
    with open(os.path.join(d, "toobig.txt"), "w") as f:   # the second record's value is one more than a short holds
        f.write("x,y,value\n%r,%r,5\n%r,%r,32768\n" % (gt[0] + 1.0, gt[3] - 1.0, gt[0] + 1.0, gt[3] - 1.0))


def runs(kind):
    if kind == "err":
        return [("err/editraster/missing_raster", ["-in", "@nope", "-out", ">out.tif", "-changes", "@@dup.txt"], 1),
                ("err/editraster/missing_changes", ["-in", "@in", "-out", ">out.tif", "-changes", "@@nope.txt"], 1),
                ("err/editraster/value_outside_int16", ["-in", "@in", "-out", ">out.tif", "-changes", "@@toobig.txt"], 1)]
    return [(f"gpu{gpus}/wide/editraster/{name}", ["-in", "@in", "-out", ">out.tif", "-changes", f"@@{name}.txt"], gpus) for gpus in (1, 3) for name in ("edges", "dup")]


def collect(kind):
    tt = _tt()
    got = {}
    with tempfile.TemporaryDirectory(prefix="tdx_editraster_transcripts_") as d:
        d = os.path.realpath(d)
        indir = os.path.join(d, "wide")
        write_inputs(indir)
        for rid, args, gpus in runs(kind):
            got[rid] = t = tt.run_one(d, rid.replace("/", "_"), indir, "editraster", args, gpus)
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
