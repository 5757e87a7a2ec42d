"""Golden vectors of the five late sweep tools - RetLimFlow, DinfAvalanche, FlowDirCond, D8VDistToStrm, SlopeAveDown - on the reduced
pathological inputs of make_golden_pathological.py: runs the REAL reference tools on the reference's own fel / p / ang of the committed
patho_<case>.npz.  Build container only, after build() has left the reference's common objects in oracle/_ref/obj:

    python tests/golden/make_golden_patholate.py

The five tools are compiled into a temporary directory (make_golden_d8rev.build_tool: the flags of oracle/Makefile's REFFLAGS, linked
against oracle/_ref/obj); nothing is written under oracle/.  patholate_<case>.npz holds
  * the new inputs, drawn by tests/downstream.extras_late (seed 40 + case index, values on grids of 1/8 and 1/16): in_wg, in_rc, in_z, the
    chosen source cells in_ass (in_ass_direct where the -direct runs get one source cell of their own, `direct` says which), and in_ang_a:
    the REFERENCE's DinfFlowDir angles of fel on the avalanche's 30 x 40 cells (30 x 30 for every other tool, as in patho_<case>.npz);
  * the reference's rasters under the keys of tests/downstream.reference_late: qrl, zfdc, vd / vd_none / vd_ad8, slpd_a / slpd_b, rz / dfs
    for path and -direct mode at both (thresh, alpha) pairs; geo = {xleftedge, ytopedge, dlon, dlat} of the avalanche's files; the libc
    that evaluated the reference's float atan.
The files are named patholate_*.npz: patho_fixture.names() globs patho_*.npz and does not match them; patho_*.npz are only read.  The
script prints, per avalanche run, the cells with rz data and the share the restatement marks as tainted.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aval_model  # noqa: E402
import downstream as D  # noqa: E402
import patho_fixture as F  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from golden.make_golden_d8rev import build_tool  # noqa: E402
from golden.make_golden_pathological import CASES  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
DX = DY = 30.0
FLT_ND = -3.402823466e38


def make(exes, R, i, name):
    inp = F.inputs(F.load(name))
    ny, nx = inp["p"].shape
    adx, ady = D.PYTH
    gt = (1000.0, DX, 0.0, 5000.0 + DY * ny, 0.0, -DY)
    agt = (1000.0, adx, 0.0, 5000.0 + ady * ny, 0.0, -ady)
    res = {"index": np.int32(i), "geo": np.array([agt[0], agt[3], adx, ady], np.float64), "libc": np.array(aval_model.libc_tag())}
    with tempfile.TemporaryDirectory() as d:
        f = lambda s: os.path.join(d, s)  # noqa: E731

        def put(key, a, nodata, g=gt):
            T.write_raster(f(key + ".tif"), a, nodata, geotransform=g)
            return f(key + ".tif")

        def ref(tool, args, outs):
            O.run_ref(exes.get(tool, tool), args)
            for k in outs:
                res[k] = T.read_raster(f(k + ".tif"), np.float32)[0]

        # the avalanche's angles: the reference's DinfFlowDir on the 30 x 40 files
        put("afel", inp["fel"], D.FEL_ND, agt)
        O.run_ref("dinfflowdir", ["-fel", f("afel.tif"), "-ang", f("ang_a.tif"), "-slp", f("slp_a.tif")])
        inp["ang_a"] = T.read_raster(f("ang_a.tif"), np.float32)[0]
        inp["aval_geo"] = tuple(float(v) for v in res["geo"])
        D.extras_late(inp, 40 + i, R, DX, DY, i, direct=D.LATE_DIRECT.get(name, "scattered"))
        inp["aval_geo"] = tuple(float(v) for v in res["geo"])       # (extras_late set the default geometry: the files' is the one the reference reads)
        res["direct"] = np.array(inp["aval_direct"])
        for k in ("wg", "rc", "z", "ass", "ang_a") + (("ass_direct",) if "ass_direct" in inp else ()):
            res["in_" + k] = inp[k]
        put("ang", inp["ang"], D.ANG_ND)
        put("p", inp["p"], D.P_ND)
        put("wg", inp["wg"], D.WG_ND)
        put("rc", inp["rc"], D.RC_ND)
        put("z", inp["z"], D.FEL_ND)
        put("feld", inp["feld"], D.FEL_ND)
        for k in ("src32", "src32_none", "ad8i"):
            put(k, inp[k], D.SRC_ND)
        ref("retlimflow", ["-ang", f("ang.tif"), "-wg", f("wg.tif"), "-rc", f("rc.tif"), "-qrl", f("qrl.tif")], ["qrl"])
        Pp = ["-p", f("p.tif")]
        ref("flowdircond", Pp + ["-z", f("z.tif"), "-zfdc", f("zfdc.tif")], ["zfdc"])
        V = Pp + ["-fel", f("feld.tif")]
        ref("d8vdisttostrm", V + ["-src", f("src32.tif"), "-dist", f("vd.tif")], ["vd"])
        ref("d8vdisttostrm", V + ["-src", f("src32_none.tif"), "-dist", f("vd_none.tif")], ["vd_none"])
        ref("d8vdisttostrm", V + ["-src", f("ad8i.tif"), "-thresh", "40", "-dist", f("vd_ad8.tif")], ["vd_ad8"])
        for k, dn, niter in D.late_dns(DX, DY, i):
            _, err, _ = O.run_ref(exes["slopeavedown"], V + ["-dn", repr(float(dn)), "-slpd", f(k + ".tif")])
            assert f"interations to do {niter}" in err, (k, err[-300:])
            res[k] = T.read_raster(f(k + ".tif"), np.float32)[0]
        put("aang", inp["ang_a"], D.ANG_ND, agt)
        put("afeld", inp["feld"], D.FEL_ND, agt)
        put("ass", inp["ass"], aval_model.ASS_NODATA, agt)
        if "ass_direct" in inp:
            put("ass_direct", inp["ass_direct"], aval_model.ASS_NODATA, agt)
        note = []
        for sfx, direct, (thresh, alpha), ass in D._aval_inputs(inp):
            assf = f("ass_direct.tif") if direct and "ass_direct" in inp else f("ass.tif")
            ref("dinfavalanche", ["-ang", f("aang.tif"), "-fel", f("afeld.tif"), "-ass", assf, "-rz", f(f"rz{sfx}.tif"), "-dfs", f(f"dfs{sfx}.tif"), "-thresh", str(thresh),
                                  "-alpha", str(alpha)] + (["-direct"] if direct else []), ["rz" + sfx, "dfs" + sfx])
            rz, dfs, taint = D._aval_ref(R, inp, ass, direct, (thresh, alpha))
            has = int((res["rz" + sfx] > -1e30).sum())
            same = np.array_equal(rz.view(np.uint32), res["rz" + sfx].view(np.uint32)) and np.array_equal(dfs.view(np.uint32), res["dfs" + sfx].view(np.uint32))
            note.append(f"{sfx[1:]} {has} cells, tainted {taint.sum() / max(has, 1):.4f}, restatement {'same' if same else 'DIFFERENT'}")
            assert taint.sum() <= aval_model.MAX_TAINT_SHARE * max(has, 1), "too many tainted cells: choose other sources"
    np.savez_compressed(os.path.join(OUT, f"patholate_{name}.npz"), **res)
    print(name, (ny, nx), f"-direct sources: {inp['aval_direct']};", "; ".join(note), "; file bytes", os.path.getsize(os.path.join(OUT, f"patholate_{name}.npz")))


if __name__ == "__main__":
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exes = {"retlimflow": build_tool(tmp, "retlimflow", ("RetlimFlow", "RetLimFlowmn")),
                "dinfavalanche": build_tool(tmp, "dinfavalanche", ("DinfAvalanche", "DinfAvalanchemn")),
                "flowdircond": build_tool(tmp, "flowdircond", ("flowdircond", "flowdirconditionmn")),
                "d8vdisttostrm": build_tool(tmp, "d8vdisttostrm", ("D8VDistToStrm", "D8VDistToStrmmn")),
                "slopeavedown": build_tool(tmp, "slopeavedown", ("SlopeAveDown", "SlopeAveDownmn"))}
        R = D.Restate(tmp, O)
        for i, name in enumerate(CASES):
            make(exes, R, i, name)
