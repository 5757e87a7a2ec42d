"""Golden vectors for CatchHydroGeo (src/CatchHydroGeo.cpp) and InunDepth (src/InunDepth.cpp): runs the REAL reference tools on a HAND raster of
the committed cases.  Build container only, after build() has left the reference's common objects in oracle/_ref/obj:

    python tests/golden/make_golden_hand.py

The reference tools are compiled into a temporary directory with make_golden_d8rev.build_tool; nothing is written under oracle/.
hand_<case>.npz holds
  * the inputs: hand = dd_ave_v of distdown_<case>.npz (dinfdistdown -m ave v) with 8 cells forced to exactly 0, 2 to +5e-7, 2 to -5e-7 and 6
    to nodata; slp of case_<case>.npz with 5 nodata cells; catch: Voronoi labels of 9 seeds with the ids CATCH_IDS, 1 % nodata cells (two of the
    ids are not in the list); mask (int16, 0 / 1 / nodata); per-row cell sizes; the geotransform;
  * the text inputs as bytes: list_csv (a duplicated id, an id the raster does not have, a zero length; three columns for `rect_dxdy`, four
    elsewhere), stages_txt (12 stages and a negative one, unsorted, one repeated, one 0), fc_csv (flows below, above, inside and exactly on the
    table, an id without rows, a depth <= 0, a repeated id);
  * table_txt: catchhydrogeo -table; map, depth_csv: inundepth -inun -depth; map_mask, depth_csv_mask: the same with -mask;
  * for `plain` and `geographic`: table_txt_3, map_3, depth_csv_3 from 3 ranks.  Whether they equal the 1-rank outputs is printed, not
    asserted: the float inundated-area sum depends on the rank order.
The files are named hand_*.npz, not case_*.npz: conftest.golden_cases() takes every case_*.npz as a case.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import hand_model as M  # noqa: E402
import make_golden_d8rev as R  # noqa: E402  (build_tool)
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = R.CASES
CATCH_IDS = (7, -5, 1200, 33, -12, 90210, 5, 64, 400)          # 64 and 400 are not in the list
#            id     slope     length  n
LIST_ROWS = ((7, 0.0123456789, 310.0, 0.035), (-5, 0.002, 120.5, 0.05), (1200, 0.03, 95.25, 0.1), (33, 0.0004, 800.0, 0.04), (7, 0.011, 275.0, 0.06),
             (-12, 0.02, 150.0, 0.045), (90210, 0.007, 410.0, 0.05), (5, 0.01, 0.0, 0.05), (999, 0.01, 100.0, 0.05))
STAGES = (-0.25, 0.5, 0.0, 1.0, 2.0, 1.0, 3.0, 5.0, 4.0, 8.0, 12.0, 20.0, 40.0)


def as_bytes(s):
    return np.frombuffer(s if isinstance(s, bytes) else s.encode(), np.uint8).copy()


def inputs(name):
    g = np.load(os.path.join(OUT, f"case_{name}.npz"))
    dd = np.load(os.path.join(OUT, f"distdown_{name}.npz"))
    hand = dd["dd_ave_v"].astype(np.float32).copy()
    ny, nx = hand.shape
    rng = np.random.default_rng(9100 + nx + ny)
    valued = np.flatnonzero(hand > -1e30)
    pick = rng.choice(valued, 18, replace=False)
    hand.flat[pick[:8]] = 0.0
    hand.flat[pick[8:10]] = 5e-7
    hand.flat[pick[10:12]] = -5e-7
    hand.flat[pick[12:]] = M.HAND_NODATA
    slp = g["slp"].astype(np.float32).copy()
    slp.flat[rng.choice(valued, 5, replace=False)] = M.SLP_NODATA
    cat = M.voronoi(ny, nx, len(CATCH_IDS), 9200 + nx, CATCH_IDS)
    cat.flat[np.flatnonzero(rng.random(ny * nx) < 0.01)] = M.CATCH_NODATA
    mask = (rng.random((ny, nx)) < 0.3).astype(np.int16)
    mask.flat[np.flatnonzero(rng.random(ny * nx) < 0.4)] = M.MASK_NODATA
    return g, hand, slp, cat, mask


def list_text(three):
    head = "id,slope,length\n" if three else "id,slope,length,n\n"
    return head + "".join(f"{i},{s!r},{ln!r}\n" if three else f"{i},{s!r},{ln!r},{n!r}\n" for i, s, ln, n in LIST_ROWS)


def forecasts(table_text):
    """Flows chosen from the table the reference wrote (columns 1, 2, 14 as float32, as InunDepth reads them)."""
    rows = [ln.split(",") for ln in table_text.strip().split("\n")[1:]]
    flows = {}
    for r in rows:
        flows.setdefault(int(r[0]), []).append(float(np.float32(float(r[13]))))
    pos = {i: [q for q in v if q > 0] for i, v in flows.items()}
    inside = lambda i: 0.5 * (sorted(pos[i])[len(pos[i]) // 2 - 1] + sorted(pos[i])[len(pos[i]) // 2])  # noqa: E731
    fc = [(7, inside(7) * 1.7), (-5, -1.0), (1200, 10.0 * max(flows[1200]) + 1.0), (33, sorted(pos[33])[1]), (31337, 5.0),
          (-12, min(pos[-12]) / 10.0), (90210, inside(90210)), (7, inside(7)), (5, 1.0)]
    return "id,flow\n" + "".join(f"{i},{q!r}\n" for i, q in fc)


def make(exes, name, ranks3=False):
    g, hand, slp, cat, mask = inputs(name)
    ny, nx = hand.shape
    dx, dy, geographic = float(g["dx"]), float(g["dy"]), bool(g["geographic"])
    gt = (-111.9, dx, 0.0, 41.9, 0.0, -dy) if geographic else (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)
    res = {"hand": hand, "slp": slp, "catch": cat, "mask": mask, "dxc": g["dxc"], "dyc": g["dyc"], "gt": np.array(gt), "geographic": np.bool_(geographic)}
    with tempfile.TemporaryDirectory() as d:
        f = lambda s: os.path.join(d, s)  # noqa: E731
        T.write_raster(f("hand.tif"), hand, M.HAND_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("slp.tif"), slp, M.SLP_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("catch.tif"), cat, M.CATCH_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("mask.tif"), mask, M.MASK_NODATA, geotransform=gt, geographic=geographic)
        open(f("list.csv"), "w").write(list_text(name == "rect_dxdy"))
        open(f("stages.txt"), "w").write("Stage\n" + "".join(f"{s!r}\n" for s in STAGES))
        chg = ["-hand", f("hand.tif"), "-catch", f("catch.tif"), "-catchlist", f("list.csv"), "-slp", f("slp.tif"), "-h", f("stages.txt")]
        O.run_ref(exes["chg"], chg + ["-table", f("table.txt")])
        table = open(f("table.txt")).read()
        open(f("fc.csv"), "w").write(forecasts(table))
        inun = ["-hand", f("hand.tif"), "-catch", f("catch.tif"), "-fc", f("fc.csv"), "-hp", f("table.txt")]
        O.run_ref(exes["inun"], inun + ["-inun", f("map.tif"), "-depth", f("depth.csv")])
        O.run_ref(exes["inun"], inun + ["-mask", f("mask.tif"), "-inun", f("map_mask.tif"), "-depth", f("depth_mask.csv")])
        for key in ("list.csv", "stages.txt", "fc.csv", "table.txt", "depth.csv", "depth_mask.csv"):
            res[key.replace(".", "_").replace("depth_mask_csv", "depth_csv_mask")] = as_bytes(open(f(key), "rb").read())
        res["map"], _ = T.read_raster(f("map.tif"), np.float32)
        res["map_mask"], _ = T.read_raster(f("map_mask.tif"), np.float32)
        same = ""
        if ranks3:
            O.run_ref(exes["chg"], chg + ["-table", f("table3.txt")], 3)
            O.run_ref(exes["inun"], ["-hand", f("hand.tif"), "-catch", f("catch.tif"), "-fc", f("fc.csv"), "-hp", f("table3.txt"), "-inun", f("map3.tif"), "-depth",
                                     f("depth3.csv")], 3)
            res["table_txt_3"] = as_bytes(open(f("table3.txt"), "rb").read())
            res["depth_csv_3"] = as_bytes(open(f("depth3.csv"), "rb").read())
            res["map_3"], _ = T.read_raster(f("map3.tif"), np.float32)
            same = "  3 ranks vs 1 rank: " + "; ".join(f"{k}: {'same' if a else 'DIFFERENT'}" for k, a in (
                ("table", bytes(res["table_txt_3"]) == bytes(res["table_txt"])), ("depth csv", bytes(res["depth_csv_3"]) == bytes(res["depth_csv"])),
                ("map", np.array_equal(res["map_3"].view(np.uint32), res["map"].view(np.uint32)))))
    np.savez_compressed(os.path.join(OUT, f"hand_{name}.npz"), **res)
    print(name, hand.shape, "map valued", int((res["map"] > -1e30).sum()), "map_mask valued", int((res["map_mask"] > -1e30).sum()))
    print(bytes(res["depth_csv"]).decode())
    if same:
        print(same)


if __name__ == "__main__":
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exes = {"chg": R.build_tool(tmp, "catchhydrogeo", ("CatchHydroGeo", "CatchHydroGeomn")), "inun": R.build_tool(tmp, "inundepth", ("InunDepth", "InunDepthmn"))}
        for c in CASES:
            make(exes, c, ranks3=c in ("plain", "geographic"))
