"""Transcripts of the two HAND tools, in the form of scripts/tool_transcripts.py (whose run_one / differences / normalisation are used): exit
status, stdout and stderr with times blanked, SHA-256 of every output file, for bin/catchhydrogeo and bin/inundepth on the `plain` golden with
--gpus 1 and --gpus 2 (InunDepth also with -mask), and two error runs that need no GPU.

    python scripts/hand_transcripts.py --record tests/golden/tool_transcripts_hand.json     (on a GPU machine)
    python scripts/hand_transcripts.py --check tests/golden/tool_transcripts_hand.json [--kind err|gpu]
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
    import hand_model as M
    import taudem_amd as T

    g = M.load_golden("plain")
    os.makedirs(d, exist_ok=True)
    gt, geo = tuple(g["gt"]), bool(g["geographic"])
    for name, key, nd in (("hand", "hand", M.HAND_NODATA), ("slp", "slp", M.SLP_NODATA), ("catch", "catch", M.CATCH_NODATA), ("mask", "mask", M.MASK_NODATA)):
        T.write_raster(os.path.join(d, name + ".tif"), g[key], nd, geotransform=gt, geographic=geo)
    for key, name in (("list_csv", "list.csv"), ("stages_txt", "stages.txt"), ("fc_csv", "fc.csv"), ("table_txt", "table.txt")):
        open(os.path.join(d, name), "wb").write(M.text_of(g[key]))
    open(os.path.join(d, "two.csv"), "w").write("id,slope\n7,0.01\n")


CHG = ["-hand", "@hand", "-catch", "@catch", "-catchlist", "@@list.csv", "-slp", "@slp", "-h", "@@stages.txt", "-table", ">table.txt"]
INUN = ["-hand", "@hand", "-catch", "@catch", "-fc", "@@fc.csv", "-hp", "@@table.txt", "-inun", ">map.tif", "-depth", ">depth.csv"]


def runs(kind):
    if kind == "err":
        return [("err/catchhydrogeo/no_list", "catchhydrogeo", [a.replace("@@list.csv", "@@missing.csv") for a in CHG], 1),
                ("err/catchhydrogeo/two_columns", "catchhydrogeo", [a.replace("@@list.csv", "@@two.csv") for a in CHG], 1)]
    out = []
    for gpus in (1, 2):
        out.append((f"gpu{gpus}/plain/catchhydrogeo/base", "catchhydrogeo", CHG, gpus))
        out.append((f"gpu{gpus}/plain/inundepth/depth", "inundepth", INUN, gpus))
    out.append(("gpu1/plain/inundepth/mask", "inundepth", INUN[:4] + ["-mask", "@mask"] + INUN[4:], 1))
    return out


def collect(kind):
    tt = _tt()
    got = {}
    with tempfile.TemporaryDirectory(prefix="tdx_hand_transcripts_") as d:
        d = os.path.realpath(d)
        indir = os.path.join(d, "plain")
        write_inputs(indir)
        for rid, tool, args, gpus in runs(kind):
            t = tt.run_one(d, rid.replace("/", "_"), indir, tool, args, gpus)
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
