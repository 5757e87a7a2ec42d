#!/usr/bin/env python3
"""Transcripts of the 22 command-line tools: exit status, stdout, stderr and the SHA-256 of every output file, for one fixed set of
runs on rasters of tests/golden/*.npz.  A refactor of the file-level tool functions (taudem_amd/csrc/capi_tools.cpp) has to
reproduce them entry for entry.

  scripts/tool_transcripts.py --record tests/golden/tool_transcripts.json [--kind err|gpu]   (on a build of the commit to compare against)
  scripts/tool_transcripts.py --check  tests/golden/tool_transcripts.json [--kind err|gpu]

kind "gpu": every tool with --gpus 1 and --gpus 3 on the `plain` case (every optional branch: -o, -wg, masks, -nc, -cs, the four
            distance types, -direct), the tools that take cell sizes on the `geographic` case, and every tool once on one GPU with
            TAUDEM_AMD_STATS=1: which tools print a statistics line, and under which name.  All of these end with status 0; the
            first one that does not (a signal, an abort, a time limit, any error) is the last one started.
kind "err": runs that return before a GPU context is created, so they need no GPU: a missing first input per tool, an input of
            another size at every comparison site, and the early exits (-sfdr, -upid, a negative -dn, a type out of range).
Numbers after "time: " and the statistics line's device time, rate and round count become T, a run's output directory becomes $O
and the scratch directory $D."""
import argparse
import concurrent.futures
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "taudem_amd", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")
ANG_ND, FEL_ND = -3.402823466e38, -3.0e38
TOOLS = ("pitremove d8flowdir aread8 dinfflowdir areadinf dinfdecayaccum gridnet threshold d8flowpathextremeup dinfupdependence dinfrevaccum "
         "dinfdistdown dinfdistup d8hdisttostrm d8vdisttostrm gagewatershed flowdircond slopeavedown dinfconclimaccum dinftranslimaccum "
         "retlimflow dinfavalanche").split()


def _npz(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def write_inputs(d, case):
    """The input rasters of every tool family for golden case `case`, under directory d; returns the scalars the runs need."""
    import taudem_amd as T

    os.makedirs(d, exist_ok=True)
    c, fa, gn = _npz(f"case_{case}"), _npz(f"case_{case}_flowalg"), _npz(f"case_{case}_gridnet")
    dd, du, av, rv, la = _npz(f"distdown_{case}"), _npz(f"distup_{case}"), _npz(f"aval_{case}"), _npz(f"d8rev_{case}"), _npz(f"d8last_{case}")
    ny = c["dem"].shape[0]
    dx, dy, geo = float(c["dx"]), float(c["dy"]), bool(c["geographic"])
    gt = (-111.9, dx, 0.0, 41.9, 0.0, -dy) if geo else (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)

    def w(name, a, nodata, gt_=gt):
        T.write_raster(os.path.join(d, name + ".tif"), np.ascontiguousarray(a), nodata, geotransform=gt_, geographic=geo)

    w("dem", c["dem"], float(c["nodata"])); w("fel", c["fel"], FEL_ND); w("p", c["p"], -32768); w("ang", c["ang"], ANG_ND)
    w("w", c["w"], -9999.0); w("dm", c["dm"], -9999.0); w("ad8", c["ad8_nc"], -1.0)
    w("dg", fa["dg"], -2147483647); w("wg", fa["wg"], -9999.0); w("dm2", fa["dm2"], -9999.0); w("q", fa["q"], -9999.0)
    w("dgs", fa["dgs"], -32768); w("tsup", fa["tsup"], -9999.0); w("tc", fa["tc"], -9999.0); w("cs", fa["cs"], -9999.0)
    w("mask", gn["mask_i32"], -2147483647); w("tmask", gn["tmask"], -1.0)
    w("dd_ang", dd["ang"], ANG_ND); w("dd_fel", dd["fel"], FEL_ND); w("dd_src", dd["src"], int(dd["src_nodata"])); w("dd_wg", dd["wg"], -9999.0)
    w("du_ang", du["ang"], ANG_ND); w("du_fel", du["fel"], FEL_ND); w("du_wg", du["wg"], -9999.0)
    xl, yt, adx, ady = (float(v) for v in av["geo"])
    agt = (xl, adx, 0.0, yt, 0.0, -ady)
    w("av_ang", av["ang"], ANG_ND, agt); w("av_fel", av["fel"], FEL_ND, agt); w("av_wg", av["wg"], -9999.0, agt); w("av_rc", av["rc"], -9999.0, agt)
    w("av_ass", av["ass"], -32768, agt)
    rgt = tuple(float(v) for v in rv["gt"])
    w("r_p", rv["p"], -32768, rgt); w("r_src", rv["src"].astype(np.int16), int(rv["src_nodata"]), rgt); w("r_ad8", rv["ad8"], int(rv["ad8_nodata"]), rgt)
    lgt, lnd = tuple(float(v) for v in la["gt"]), float(la["fel_nodata"])
    w("l_p", la["p"], -32768, lgt); w("l_fel", la["fel"], lnd, lgt); w("l_z", la["z"], lnd, lgt); w("l_src", la["src"].astype(np.int16), int(la["src_nodata"]), lgt)
    w("small", c["fel"][:-3, :-5], FEL_ND)   # another size: the readers convert to the type asked for, so one file serves every site
    with open(os.path.join(d, "outlets.txt"), "w") as fo:
        for x_, y_ in zip(*c["outlet_xy"]):
            fo.write(f"{float(x_)!r} {float(y_)!r}\n")
    with open(os.path.join(d, "gauges.txt"), "w") as fo:
        for col, row, i in zip(rv["cols"], rv["rows"], rv["ids"]):
            fo.write(f"{float(rgt[0] + (col + 0.5) * rgt[1])!r} {float(rgt[3] - (row + 0.5) * -rgt[5])!r} {i}\n")
    return {"gn_thresh": str(int(gn["gn_thresh"])), "ssa_thresh": str(float(gn["ssa_thresh"])), "dn": repr(float(la["dn"][1]))}


# One run: (tool, tag, args).  In args "@name" is the input raster name.tif, "@@name" another input file, ">name" an output file.
def tool_runs(k):
    o = ["-o", "@@outlets.txt"]
    ddb = ["-ang", "@dd_ang", "-fel", "@dd_fel", "-slp", "@never_read", "-src", "@dd_src", "-dd", ">dd.tif"]
    dub = ["-ang", "@du_ang", "-fel", "@du_fel", "-slp", "@never_read", "-du", ">du.tif"]
    cl = ["-ang", "@ang", "-dg", "@dgs", "-dm", "@dm2", "-q", "@q", "-ctpt", ">ctpt.tif"]
    tl = ["-ang", "@ang", "-tsup", "@tsup", "-tc", "@tc", "-tla", ">tla.tif", "-tdep", ">tdep.tif"]
    return [
        ("pitremove", "", ["-z", "@dem", "-fel", ">fel.tif"]),
        ("pitremove", "v_4way", ["-z", "@dem", "-fel", ">fel.tif", "-v", "-4way"]),
        ("pitremove", "depmask_v", ["-z", "@dem", "-fel", ">fel.tif", "-depmask", "@dgs", "-v"]),
        ("d8flowdir", "", ["-fel", "@fel", "-p", ">p.tif", "-sd8", ">sd8.tif"]),
        ("dinfflowdir", "", ["-fel", "@fel", "-ang", ">ang.tif", "-slp", ">slp.tif"]),
        ("aread8", "", ["-p", "@p", "-ad8", ">ad8.tif"]),
        ("aread8", "wg_nc", ["-p", "@p", "-ad8", ">ad8.tif", "-wg", "@w", "-nc"]),
        ("aread8", "o", ["-p", "@p", "-ad8", ">ad8.tif", *o]),
        ("areadinf", "", ["-ang", "@ang", "-sca", ">sca.tif"]),
        ("areadinf", "wg_nc", ["-ang", "@ang", "-sca", ">sca.tif", "-wg", "@w", "-nc"]),
        ("areadinf", "o_nc", ["-ang", "@ang", "-sca", ">sca.tif", *o, "-nc"]),
        ("dinfdecayaccum", "", ["-ang", "@ang", "-dm", "@dm", "-dsca", ">dsca.tif"]),
        ("dinfdecayaccum", "wg_nc", ["-ang", "@ang", "-dm", "@dm", "-dsca", ">dsca.tif", "-wg", "@w", "-nc"]),
        ("dinfdecayaccum", "o_nc", ["-ang", "@ang", "-dm", "@dm", "-dsca", ">dsca.tif", *o, "-nc"]),
        ("gridnet", "", ["-p", "@p", "-plen", ">plen.tif", "-tlen", ">tlen.tif", "-gord", ">gord.tif"]),
        ("gridnet", "mask", ["-p", "@p", "-plen", ">plen.tif", "-tlen", ">tlen.tif", "-gord", ">gord.tif", "-mask", "@mask", "-thresh", k["gn_thresh"]]),
        ("gridnet", "o", ["-p", "@p", "-plen", ">plen.tif", "-tlen", ">tlen.tif", "-gord", ">gord.tif", *o]),
        ("threshold", "", ["-ssa", "@ad8", "-src", ">src.tif", "-thresh", k["ssa_thresh"]]),
        ("threshold", "mask", ["-ssa", "@ad8", "-src", ">src.tif", "-thresh", k["ssa_thresh"], "-mask", "@tmask"]),
        ("d8flowpathextremeup", "", ["-p", "@p", "-sa", "@ad8", "-ssa", ">ssa.tif"]),
        ("d8flowpathextremeup", "min_nc", ["-p", "@p", "-sa", "@ad8", "-ssa", ">ssa.tif", "-min", "-nc"]),
        ("d8flowpathextremeup", "o_nc", ["-p", "@p", "-sa", "@ad8", "-ssa", ">ssa.tif", *o, "-nc"]),
        ("dinfupdependence", "", ["-ang", "@ang", "-dg", "@dg", "-dep", ">dep.tif"]),
        ("dinfrevaccum", "", ["-ang", "@ang", "-wg", "@wg", "-racc", ">racc.tif", "-dmax", ">dmax.tif"]),
        ("dinfconclimaccum", "", cl),
        ("dinfconclimaccum", "o_nc", [*cl, *o, "-nc"]),
        ("dinftranslimaccum", "", tl),
        ("dinftranslimaccum", "cs_nc", [*tl, "-cs", "@cs", "-ctpt", ">ctpt.tif", "-nc"]),
        ("dinftranslimaccum", "cs_o_nc", [*tl, "-cs", "@cs", "-ctpt", ">ctpt.tif", *o, "-nc"]),
        ("dinfdistdown", "ave_h", [*ddb, "-m", "ave", "h"]),
        ("dinfdistdown", "max_v", [*ddb, "-m", "v", "max"]),
        ("dinfdistdown", "min_p_wg", [*ddb, "-m", "min", "p", "-wg", "@dd_wg"]),
        ("dinfdistdown", "ave_s_nc", [*ddb, "-m", "ave", "s", "-nc"]),
        ("dinfdistup", "ave_h", [*dub, "-m", "ave", "h"]),
        ("dinfdistup", "max_v", [*dub, "-m", "v", "max"]),
        ("dinfdistup", "min_p_wg", [*dub, "-m", "min", "p", "-wg", "@du_wg"]),
        ("dinfdistup", "ave_s_nc", [*dub, "-m", "ave", "s", "-nc"]),
        ("dinfdistup", "ave_h_thresh", [*dub, "-m", "ave", "h", "-thresh", "0.3"]),
        ("retlimflow", "", ["-ang", "@av_ang", "-wg", "@av_wg", "-rc", "@av_rc", "-qrl", ">qrl.tif"]),
        ("dinfavalanche", "", ["-ang", "@av_ang", "-fel", "@av_fel", "-ass", "@av_ass", "-rz", ">rz.tif", "-dfs", ">dfs.tif"]),
        ("dinfavalanche", "direct", ["-ang", "@av_ang", "-fel", "@av_fel", "-ass", "@av_ass", "-rz", ">rz.tif", "-dfs", ">dfs.tif", "-direct"]),
        ("d8hdisttostrm", "", ["-p", "@r_p", "-src", "@r_src", "-dist", ">dist.tif"]),
        ("d8hdisttostrm", "thresh", ["-p", "@r_p", "-src", "@r_ad8", "-thresh", "40", "-dist", ">dist.tif"]),
        ("d8vdisttostrm", "", ["-p", "@l_p", "-fel", "@l_fel", "-src", "@l_src", "-dist", ">dist.tif"]),
        ("gagewatershed", "id", ["-p", "@r_p", "-o", "@@gauges.txt", "-gw", ">gw.tif", "-id", ">id.txt"]),
        ("flowdircond", "", ["-p", "@l_p", "-z", "@l_z", "-zfdc", ">zfdc.tif"]),
        ("slopeavedown", "", ["-p", "@l_p", "-fel", "@l_fel", "-slpd", ">slpd.tif", "-dn", k["dn"]]),
    ]


GEOGRAPHIC_TAGS = {("d8flowdir", ""), ("dinfflowdir", ""), ("gridnet", "o"), ("areadinf", ""), ("dinfdistdown", "ave_s_nc"), ("dinfdistup", "min_p_wg"),
                   ("dinfavalanche", "direct"), ("d8hdisttostrm", ""), ("slopeavedown", ""), ("dinfrevaccum", "")}


def error_runs(k):
    """(tool, tag, args) of the runs that end before a GPU context exists."""
    runs = []
    base = {}
    for tool, tag, args in tool_runs(k):   # per tool, the variant that reads the most files
        if tool not in base or sum(a.startswith("@") for a in args) > sum(a.startswith("@") for a in base[tool]):
            base[tool] = args
    for tool in TOOLS:
        args = base[tool]
        rasters = [i for i, a in enumerate(args) if a.startswith("@") and not a.startswith("@@") and a != "@never_read"]
        runs.append((tool, "missing", [("@nope" if i in rasters else a) for i, a in enumerate(args)]))
        first = rasters[0] if tool != "slopeavedown" else rasters[1]   # (SlopeAveDown reads fel first)
        for i in rasters:
            if i != first:
                runs.append((tool, "small_" + args[i][1:], [("@small" if j == i else a) for j, a in enumerate(args)]))
    # the distance tools read fel only for v / p / s and the weight only for h / p / s: p covers both above; h and v each skip one
    runs.append(("dinfdistdown", "h_small_fel_not_read_small_src", ["-ang", "@dd_ang", "-fel", "@small", "-slp", "@never_read", "-src", "@small", "-dd", ">dd.tif", "-m", "ave", "h"]))
    runs.append(("dinfdistup", "v_small_wg_not_read_small_fel", ["-ang", "@du_ang", "-fel", "@small", "-slp", "@never_read", "-wg", "@small", "-du", ">du.tif", "-m", "ave", "v"]))
    runs.append(("aread8", "missing_outlets", ["-p", "@p", "-ad8", ">ad8.tif", "-o", "@@nope.txt"]))
    runs.append(("d8flowdir", "sfdr", ["-fel", "@fel", "-p", ">p.tif", "-sd8", ">sd8.tif", "-sfdr", "@p"]))
    runs.append(("gagewatershed", "upid", ["-p", "@r_p", "-o", "@@gauges.txt", "-gw", ">gw.tif", "-upid", ">upid.txt"]))
    runs.append(("slopeavedown", "negative_dn", ["-p", "@l_p", "-fel", "@l_fel", "-slpd", ">slpd.tif", "-dn", "-1"]))
    # a distance type out of range cannot be written on the command line
    # (nor do -upid and a negative -dn get past the mains): through the library, which refuses before it opens a file
    for fn, tag, call in (("dinfdistdown", "type_out_of_range", "dinfdistdown(*['nope.tif'] * 6, typemethod=7)"),
                          ("dinfdistup", "type_out_of_range", "dinfdistup(*['nope.tif'] * 5, typemethod=7)"),
                          ("gagewatershed", "upid", "gagewatershed('nope.tif', 'gw.tif', 'nope.txt', writeupid=1, upidfile='upid.txt')"),
                          ("slopeavedown", "negative_dn", "sloped('nope.tif', 'nope.tif', 'slpd.tif', dn=-1.0)")):
        runs.append(("python:" + fn, tag, ["-c", f"import sys; from taudem_amd import tools; sys.exit(tools.{call} & 0xff)"]))
    return runs


def _sha(path):
    if not os.path.exists(path):
        return None
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _normalise(text, d, out):
    return re.sub(r'(time: |"device_ms": |"mcells_per_s": |"rounds": )[^\s,}]+', r"\1T", text.replace(out, "$O").replace(d, "$D"))


def run_one(d, run_id, indir, tool, args, gpus, stats=False):
    out = os.path.join(d, "out", run_id)
    os.makedirs(out, exist_ok=True)
    outputs, argv = [], []
    for a in args:
        if a.startswith("@@"):
            argv.append(os.path.join(indir, a[2:]))
        elif a.startswith("@") and not tool.startswith("python:"):
            argv.append(os.path.join(indir, a[1:] + ".tif"))
        elif a.startswith(">"):
            outputs.append(a[1:])
            argv.append(os.path.join(out, a[1:]))
        else:
            argv.append(a)
    env = {k_: v for k_, v in os.environ.items() if not k_.startswith("TAUDEM_AMD_")}
    if stats:
        env["TAUDEM_AMD_STATS"] = "1"
    if tool.startswith("python:"):
        cmd = [sys.executable, *argv]
        env["PYTHONPATH"] = ROOT
    else:
        cmd = [os.path.join(BIN, tool), "--gpus", str(gpus), *argv]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=d)
    shown = [_normalise(a, d, out) for a in argv] if not tool.startswith("python:") else args
    return {"argv": " ".join([tool, *(["--gpus", str(gpus)] if not tool.startswith("python:") else []), *shown]), "status": r.returncode,
            "stdout": _normalise(r.stdout, d, out), "stderr": _normalise(r.stderr, d, out), "files": {n: _sha(os.path.join(out, n)) for n in outputs}}


def collect(kind, jobs=4):
    """{run id: transcript} of the runs of `kind` ("err" or "gpu") with the tools in taudem_amd/bin."""
    with tempfile.TemporaryDirectory(prefix="tdx_transcripts_") as d:
        d = os.path.realpath(d)
        plain = os.path.join(d, "plain")
        k = write_inputs(plain, "plain")
        todo = []
        if kind == "err":
            for tool, tag, args in error_runs(k):
                todo.append((f"err/{tool}/{tag}", plain, tool, args, 1, False))
        else:
            geog = os.path.join(d, "geographic")
            kg = write_inputs(geog, "geographic")
            for gpus in (1, 3):
                for tool, tag, args in tool_runs(k):
                    todo.append((f"gpu{gpus}/plain/{tool}/{tag or 'base'}", plain, tool, args, gpus, False))
                for tool, tag, args in tool_runs(kg):
                    if (tool, tag) in GEOGRAPHIC_TAGS:
                        todo.append((f"gpu{gpus}/geographic/{tool}/{tag or 'base'}", geog, tool, args, gpus, False))
            seen = set()
            for tool, tag, args in tool_runs(k):   # each tool's first variant, with the statistics line asked for
                if tool not in seen:
                    seen.add(tool)
                    todo.append((f"gpu1/stats/{tool}/{tag or 'base'}", plain, tool, args, 1, True))
        # A GPU run that fails may have left the card in a bad state: nothing more is started on it.  The runs already under way
        # (at most jobs - 1) end by themselves; the ones not started are missing from the result, which differences() reports.
        stop = threading.Event()

        def guarded(rid, *run):
            if stop.is_set():
                return None
            try:
                t = run_one(d, rid.replace("/", "_").replace(":", "_"), *run)
            except subprocess.TimeoutExpired:
                t = {"argv": run[1], "status": "time limit", "stdout": "", "stderr": "", "files": {}}
            if kind == "gpu" and t["status"] != 0 and not stop.is_set():
                stop.set()
                print(f"{rid} ended with status {t['status']}: no further GPU run is started", file=sys.stderr)
            return t

        with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
            futs = {run[0]: ex.submit(guarded, *run) for run in todo}
            got = {rid: f.result() for rid, f in futs.items()}
        return {rid: t for rid, t in got.items() if t is not None}


def differences(expected, got):
    """Human-readable lines, one per entry of `expected` that `got` does not reproduce (and per entry only one side has)."""
    bad = []
    for rid in sorted(set(expected) | set(got)):
        e, g = expected.get(rid), got.get(rid)
        if e is None or g is None:
            bad.append(f"{rid}: {'not run (only in the fixture)' if g is None else 'only in the current build'}")
            continue
        for field in ("argv", "status", "stdout", "stderr", "files"):
            if e[field] != g[field]:
                bad.append(f"{rid}: {field} differs\n  expected: {e[field]!r}\n  got:      {g[field]!r}")
    return bad


def load_fixture(path, kind):
    with open(path) as f:
        return {rid: t for rid, t in json.load(f).items() if rid.startswith("err/") == (kind == "err")}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--record", metavar="JSON")
    ap.add_argument("--check", metavar="JSON")
    ap.add_argument("--kind", choices=["err", "gpu", "all"], default="all")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--bin", metavar="DIR", help="the tools of another build (next to its libtaudem_amd.so) instead of taudem_amd/bin")
    a = ap.parse_args()
    if a.bin:
        global BIN
        BIN = os.path.abspath(a.bin)
    kinds = ["err", "gpu"] if a.kind == "all" else [a.kind]
    got = {}
    for kind in kinds:
        got.update(collect(kind, a.jobs))
    if a.record:
        old = {}
        if os.path.exists(a.record):
            with open(a.record) as f:
                old = {rid: t for rid, t in json.load(f).items() if all(rid.startswith("err/") != (kind == "err") for kind in kinds)}
        old.update(got)
        with open(a.record, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(rid)}: {json.dumps(old[rid], sort_keys=True)}" for rid in sorted(old)) + "\n}\n")   # one run per line
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
