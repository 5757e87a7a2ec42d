"""Golden vectors for the pathological inputs (tests/pathological.py), reduced in size: runs the REAL reference tools on them, from
PitRemove down to every tool downstream of the directions.  Build container only, after build() has left the reference's tools and
common objects in oracle/_ref/:

    python tests/golden/make_golden_pathological.py

DinfDistDown, DinfDistUp, D8HDistToStrm and GageWatershed are compiled into a temporary directory (the flags of oracle/Makefile's
REFFLAGS, linked against oracle/_ref/obj); nothing is written under oracle/.  patho_<case>.npz holds
  * the DEM and the reference's fel, p, sd8, ang, slp, ad8 / ad8_nc, sca / sca_nc (30 m cells, projected);
  * the downstream tools' other inputs, drawn from the reference's rasters by tests/downstream.extras (seed 40 + case index): stream
    cells, weights, decay multipliers, supply / capacity / concentration grids, masks, outlets (x, y) and gauges (x, y, id: one on a cell
    without a direction, a second one on a taken cell, one off the raster);
  * every raster the reference wrote for them under the keys of tests/downstream.reference (the DinfDistDown / DinfDistUp -m forms
    rotate with the case index: downstream.dd_variants / du_variants), the -id file's text under gw_id.
The files are named patho_*.npz: case_*, distdown_*, distup_* and d8rev_* are globbed by other tests.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import downstream as D  # noqa: E402
import pathological as P  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from golden.make_golden_d8rev import build_tool  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
DX = DY = 30.0
CASES = {
    "plane": lambda: P.plane(60, 70),
    "ramp_shallow": lambda: P.ramp(57, 64, ax=1e-3, ay=0.0),
    "ramp_diag": lambda: P.ramp(57, 64, ax=1.0, ay=1.0),
    "checkerboard_pits": lambda: P.checkerboard_pits(56, 64),
    "spiral": lambda: P.spiral(128, 8),
    "one_row": lambda: P.one_row(700),
    "one_column": lambda: P.one_column(700),
    "two_rows": lambda: np.vstack([P.one_row(700), P.one_row(700)[:, ::-1]]),
    "all_nodata": lambda: P.all_nodata(30, 40),
    "one_data_cell": lambda: P.one_data_cell(30, 40),
    "nan_cells": lambda: P.with_specials(P.fractal(O, 56, 64), "nan", count=20),
    "+inf_cells": lambda: P.with_specials(P.fractal(O, 56, 64), "+inf", count=20),
    "-inf_cells": lambda: P.with_specials(P.fractal(O, 56, 64), "-inf", count=20),
}


def make(exes, i, name):
    dem = CASES[name]()
    ny, nx = dem.shape
    gt = (1000.0, DX, 0.0, 5000.0 + DY * ny, 0.0, -DY)
    res = {"dem": dem, "index": np.int32(i)}
    with tempfile.TemporaryDirectory() as d:
        f = lambda s: os.path.join(d, s)  # noqa: E731

        def put(key, a, nodata):
            T.write_raster(f(key + ".tif"), a, nodata, geotransform=gt)
            return f(key + ".tif")

        def get(key, dtype=np.float32):
            return T.read_raster(f(key + ".tif"), dtype)[0]

        def ref(tool, args, outs):
            O.run_ref(exes.get(tool, tool), args)
            for k, dt in outs:
                res[k] = get(k, dt)

        put("dem", dem, P.NODATA)
        ref("pitremove", ["-z", f("dem.tif"), "-fel", f("fel.tif")], [("fel", np.float32)])
        ref("d8flowdir", ["-fel", f("fel.tif"), "-p", f("p.tif"), "-sd8", f("sd8.tif")], [("p", np.int16), ("sd8", np.float32)])
        ref("dinfflowdir", ["-fel", f("fel.tif"), "-ang", f("ang.tif"), "-slp", f("slp.tif")], [("ang", np.float32), ("slp", np.float32)])
        ref("aread8", ["-p", f("p.tif"), "-ad8", f("ad8.tif")], [("ad8", np.float32)])
        ref("aread8", ["-p", f("p.tif"), "-ad8", f("ad8_nc.tif"), "-nc"], [("ad8_nc", np.float32)])
        ref("areadinf", ["-ang", f("ang.tif"), "-sca", f("sca.tif")], [("sca", np.float32)])
        ref("areadinf", ["-ang", f("ang.tif"), "-sca", f("sca_nc.tif"), "-nc"], [("sca_nc", np.float32)])
        inp = D.extras({k: res[k] for k in ("fel", "p", "sd8", "ang", "slp")} | {"ad8": res["ad8_nc"], "sca": res["sca_nc"]}, 40 + i)
        for k in ("feld", "src16", "src16_all", "w", "wpos", "dg", "dm", "q", "dgs", "tsup", "tc", "cs", "src32", "src32_none", "ad8i", "gmask", "sa",
                  "tmask"):
            res["in_" + k] = inp[k]
        res["in_outlets"] = np.stack(inp["outlets"]).astype(np.int32)
        res["in_gauges"] = np.stack(inp["gauges"]).astype(np.int32)
        nd = {"feld": -3.0e38, "src16": -32768, "src16_all": -32768, "w": -9999.0, "wpos": -9999.0, "dg": -1, "dm": -9999.0, "q": -9999.0, "dgs": -1,
              "tsup": -9999.0, "tc": -9999.0, "cs": -9999.0, "src32": D.SRC_ND, "src32_none": D.SRC_ND, "ad8i": D.SRC_ND, "gmask": -2147483647,
              "sa": -3.402823466e38, "tmask": -9999.0}
        for k, v in nd.items():
            put(k, inp[k], v)
        put("src16_none", np.zeros_like(inp["src16"]), -32768)
        with open(f("outlets.txt"), "w") as fo:
            for c, r in zip(*inp["outlets"]):
                fo.write(f"{float(gt[0] + (c + 0.5) * DX)!r} {float(gt[3] - (r + 0.5) * DY)!r}\n")
        with open(f("gauges.txt"), "w") as fo:
            for c, r, k in zip(*inp["gauges"]):
                fo.write(f"{float(gt[0] + (c + 0.5) * DX)!r} {float(gt[3] - (r + 0.5) * DY)!r} {k}\n")
        A, o = ["-ang", f("ang.tif")], ["-o", f("outlets.txt")]
        ref("dinfupdependence", A + ["-dg", f("dg.tif"), "-dep", f("dep.tif")], [("dep", np.float32)])
        ref("dinfrevaccum", A + ["-wg", f("w.tif"), "-racc", f("racc.tif"), "-dmax", f("dmax.tif")], [("racc", np.float32), ("dmax", np.float32)])
        ref("dinfdecayaccum", A + ["-dm", f("dm.tif"), "-wg", f("wpos.tif"), "-dsca", f("dsca.tif")], [("dsca", np.float32)])
        ref("dinfdecayaccum", A + ["-dm", f("dm.tif"), "-dsca", f("dsca_o.tif"), "-nc"] + o, [("dsca_o", np.float32)])
        C = A + ["-dg", f("dgs.tif"), "-dm", f("dm.tif"), "-q", f("q.tif")]
        ref("dinfconclimaccum", C + ["-ctpt", f("ctpt.tif"), "-csol", str(D.CSOL)], [("ctpt", np.float32)])
        ref("dinfconclimaccum", C + ["-ctpt", f("ctpt_o.tif"), "-nc"] + o, [("ctpt_o", np.float32)])
        L = A + ["-tsup", f("tsup.tif"), "-tc", f("tc.tif")]
        ref("dinftranslimaccum", L + ["-tla", f("tla.tif"), "-tdep", f("tdep.tif")], [("tla", np.float32), ("tdep", np.float32)])
        ref("dinftranslimaccum", L + ["-tla", f("tla_cs.tif"), "-tdep", f("tdep_cs.tif"), "-cs", f("cs.tif"), "-ctpt", f("tctpt_cs.tif"), "-nc"] + o,
            [("tla_cs", np.float32), ("tdep_cs", np.float32), ("tctpt_cs", np.float32)])
        DD = A + ["-fel", f("feld.tif"), "-slp", f("nonexistent_slp.tif")]
        wg = {"": [], "_nc": ["-nc"], "_wg": ["-wg", f("w.tif")], "_t": ["-thresh", str(D.distup_model.THRESH)]}
        for st, kd, sfx in D.dd_variants(i):
            key = f"dd_{st}_{kd}{sfx}"
            ref("dinfdistdown", DD + ["-src", f("src16.tif"), "-dd", f(key + ".tif"), "-m", st, kd] + wg[sfx], [(key, np.float32)])
        ref("dinfdistdown", DD + ["-src", f("src16_none.tif"), "-dd", f("dd_ave_h_none.tif"), "-m", "ave", "h"], [("dd_ave_h_none", np.float32)])
        ref("dinfdistdown", DD + ["-src", f("src16_all.tif"), "-dd", f("dd_min_s_all.tif"), "-m", "min", "s"], [("dd_min_s_all", np.float32)])
        for st, kd, sfx in D.du_variants(i):
            key = f"du_{st}_{kd}{sfx}"
            ref("dinfdistup", DD + ["-du", f(key + ".tif"), "-m", st, kd] + wg[sfx], [(key, np.float32)])
        Pp = ["-p", f("p.tif")]
        ref("d8hdisttostrm", Pp + ["-src", f("src32.tif"), "-dist", f("dist.tif")], [("dist", np.float32)])
        ref("d8hdisttostrm", Pp + ["-src", f("src32_none.tif"), "-dist", f("dist_none.tif")], [("dist_none", np.float32)])
        ref("d8hdisttostrm", Pp + ["-src", f("ad8i.tif"), "-thresh", "40", "-dist", f("dist_ad8.tif")], [("dist_ad8", np.float32)])
        ref("gagewatershed", Pp + ["-o", f("gauges.txt"), "-gw", f("gw.tif"), "-id", f("id.txt")], [("gw", np.int32)])
        res["gw_id"] = np.array(open(f("id.txt")).read())
        G = ["-plen", "-tlen", "-gord"]
        for sfx, extra in (("", []), ("_m", ["-mask", f("gmask.tif"), "-thresh", str(D.GN_THRESH)]), ("_o", o)):
            args = Pp + [a for g in G for a in (g, f(g[1:] + sfx + ".tif"))] + extra
            ref("gridnet", args, [("plen" + sfx, np.float32), ("tlen" + sfx, np.float32), ("gord" + sfx, np.int16)])
        S = Pp + ["-sa", f("sa.tif")]
        ref("d8flowpathextremeup", S + ["-ssa", f("xup_max.tif")], [("xup_max", np.float32)])
        ref("d8flowpathextremeup", S + ["-ssa", f("xup_min_nc.tif"), "-min", "-nc"], [("xup_min_nc", np.float32)])
        ref("d8flowpathextremeup", S + ["-ssa", f("xup_max_o.tif"), "-nc"] + o, [("xup_max_o", np.float32)])
        put("ad8f", res["ad8_nc"], -1.0)
        ref("threshold", ["-ssa", f("ad8f.tif"), "-src", f("thr.tif"), "-thresh", str(D.SSA_THRESH)], [("thr", np.int16)])
        ref("threshold", ["-ssa", f("ad8f.tif"), "-src", f("thr_m.tif"), "-thresh", str(D.SSA_THRESH), "-mask", f("tmask.tif")], [("thr_m", np.int16)])
    np.savez_compressed(os.path.join(OUT, f"patho_{name}.npz"), **res)
    print(name, dem.shape, str(res["gw_id"]).replace("\n", " | "))


if __name__ == "__main__":
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exes = {"dinfdistdown": build_tool(tmp, "dinfdistdown", ("DinfDistDown", "DinfDistDownmn")),
                "dinfdistup": build_tool(tmp, "dinfdistup", ("DinfDistUp", "DinfDistUpmn")),
                "d8hdisttostrm": build_tool(tmp, "d8hdisttostrm", ("D8HDistToStrm", "D8HDistToStrmmn")),
                "gagewatershed": build_tool(tmp, "gagewatershed", ("gagewatershed", "gagewatershedmn"))}
        for i, name in enumerate(CASES):
            make(exes, i, name)
