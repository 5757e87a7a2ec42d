"""Transcripts of bin/sinmapsi, in the form of scripts/peuker_transcripts.py (the run_one / differences / normalisation of scripts/tool_transcripts.py are
used): exit status, stdout and stderr with times blanked, SHA-256 of the two output rasters, on the `plain` run of tests/sinmap_model.py with --gpus 1 and
--gpus 2 in the three argument forms (10 positional arguments, 12 positional arguments, flags), and the error runs that end before the compute step and
need no GPU (an unreadable -calpar, a slope file that is missing, a contributing-area raster of another size).

    python scripts/sinmap_transcripts.py --record tests/golden/tool_transcripts_sinmap.json [--kind err|gpu]     (gpu: on a GPU machine; the other kind's entries are kept)
    python scripts/sinmap_transcripts.py --check tests/golden/tool_transcripts_sinmap.json [--kind err|gpu]
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
    import sinmap_model as M
    import taudem_amd as T

    r = dict(M.golden_runs("plain"))["roads"]
    os.makedirs(d, exist_ok=True)
    gt = (1000.0, 30.0, 0.0, 5000.0 + 30.0 * r["slp"].shape[0], 0.0, -30.0)
    T.write_raster(os.path.join(d, "slp.tif"), r["slp"], float(r["slp_nodata"]), geotransform=gt)
    for name in ("sca", "scamin", "scamax"):
        T.write_raster(os.path.join(d, name + ".tif"), r[name], -1.0, geotransform=gt)
    T.write_raster(os.path.join(d, "cal.tif"), r["cal"], float(r["cal_nodata"]), geotransform=gt)
    T.write_raster(os.path.join(d, "small.tif"), r["sca"][:10, :10], -1.0, geotransform=gt)
    open(os.path.join(d, "calpar.csv"), "w").write(r["calpar"])
    return [repr(M.RMINTER), repr(M.RMAXTER), repr(M.G), repr(M.RHOW)]


def runs(kind, par):
    flags = ["-slp", "@slp", "-sca", "@sca", "-calpar", "@@calpar.csv", "-cal", "@cal", "-si", ">si.tif", "-sat", ">sat.tif", "-par", *par]
    if kind == "err":
        return [("err/sinmapsi/missing_calpar", [*flags[:5], "@@nope.csv", *flags[6:]], 1), ("err/sinmapsi/missing_slp", ["-slp", "@nope", *flags[2:]], 1),
                ("err/sinmapsi/small_sca", [*flags[:3], "@small", *flags[4:]], 1)]
    pos = ["@slp", "@sca", "@@calpar.csv", "@cal", ">si.tif", ">sat.tif", *par]
    return [(f"gpu{gpus}/plain/sinmapsi/{tag}", args, gpus) for gpus in (1, 2)
            for tag, args in (("pos10", pos), ("pos12", [*pos, "@scamin", "@scamax"]), ("flags", [*flags, "-scamin", "@scamin", "-scamax", "@scamax"]))]


def collect(kind):
    tt = _tt()
    got = {}
    with tempfile.TemporaryDirectory(prefix="tdx_sinmap_transcripts_") as d:
        d = os.path.realpath(d)
        indir = os.path.join(d, "plain")
        par = write_inputs(indir)
        for rid, args, gpus in runs(kind, par):
            t = tt.run_one(d, rid.replace("/", "_"), indir, "sinmapsi", args, gpus)
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
        keep = {}
        if os.path.exists(a.record):   # entries of the kind that was not run stay
            with open(a.record) as f:
                keep = {rid: t for rid, t in json.load(f).items() if ("err" if rid.startswith("err/") else "gpu") not in kinds}
        keep.update(got)
        with open(a.record, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(rid)}: {json.dumps(keep[rid], sort_keys=True)}" for rid in sorted(keep)) + "\n}\n")
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
