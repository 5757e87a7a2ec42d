"""Golden vectors for FlowDirCond (src/flowdircond.cpp), D8VDistToStrm (src/D8VDistToStrm.cpp) and SlopeAveDown (src/SlopeAveDown.cpp): runs
the REAL reference tools on the D8 directions of the committed cases.  Build container only, after build() has left the reference's common
objects in oracle/_ref/obj:

    python tests/golden/make_golden_d8last.py

The reference tools are compiled into a temporary directory with make_golden_d8rev.build_tool (the flags of oracle/Makefile's REFFLAGS,
linked against oracle/_ref/obj); nothing is written under oracle/.  d8last_<case>.npz holds
  * the inputs: p, src and ad8 of make_golden_d8rev.inputs() (a few p == 0 cells, nodata p under stream cells, a 2-cell cycle, src nodata
    holes); fel with a few nodata cells planted under valid directions (nodata -3e38), some of them with contributors; z = fel + seeded
    normal noise of 3 m (NOT pit-filled along p: on fel itself FlowDirCond changes nothing); per-row cell sizes; the geotransform;
  * zfdc: flowdircond -p p -z z;
  * vdist_src: d8vdisttostrm -src src (default -thresh 1), vdist_ad8: -src ad8 -thresh 40;
  * dn (three distances: 0.5, 2.5 and 6.2 times the smaller cell size of the middle row, metres for the geographic case), niter (1, 3, 7)
    and slpd_0 / slpd_1 / slpd_2: slopeavedown -dn.
The reference's 3-rank runs are compared with its 1-rank runs on `holes`, `plain` and `geographic` (asserted).  The files are named
d8last_*.npz, not case_*.npz: conftest.golden_cases() takes every case_*.npz as a case.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import d8last_model as M  # noqa: E402
import make_golden_d8rev as R  # noqa: E402  (build_tool, inputs)
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = R.CASES
NOISE_M = 3.0


def inputs(name):
    g, p, src, ad8i = R.inputs(name)
    ny, nx = p.shape
    rng = np.random.default_rng(7300 + nx + ny)
    fel = g["fel"].astype(np.float32).copy()
    fel[fel < -1e30] = M.FEL_NODATA
    has_up = np.zeros((ny, nx), bool)          # cells some neighbour drains into
    for k in range(1, 9):
        ys, xs = np.nonzero(p == k)
        yn, xn = ys + R.DY_[k], xs + R.DX_[k]
        ok = (yn >= 0) & (yn < ny) & (xn >= 0) & (xn < nx)
        has_up[yn[ok], xn[ok]] = True
    inner = np.zeros((ny, nx), bool)
    inner[2:-2, 2:-2] = True
    valid = inner & (p >= 1) & (p <= 8) & (fel > -1e30)
    holes = np.concatenate([rng.choice(np.flatnonzero(valid & has_up), 6, replace=False), rng.choice(np.flatnonzero(valid & ~has_up), 3, replace=False)])
    fel.flat[holes] = M.FEL_NODATA              # nodata fel under a valid direction
    z = fel.copy()
    ok = z > -1e30
    z[ok] = (z[ok] + rng.normal(0.0, NOISE_M, int(ok.sum()))).astype(np.float32)
    return g, p, src, ad8i, fel, z


def make(exes, name, check_ranks=0):
    g, p, src, ad8i, fel, z = inputs(name)
    ny, nx = p.shape
    dx, dy, geographic = float(g["dx"]), float(g["dy"]), bool(g["geographic"])
    gt = (-111.9, dx, 0.0, 41.9, 0.0, -dy) if geographic else (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)
    dns = M.dns_of(g["dxc"], g["dyc"])
    res = {"p": p, "src": src.astype(np.int32), "src_nodata": np.int32(M.SRC_NODATA), "ad8": ad8i, "ad8_nodata": np.int32(-1), "fel": fel, "z": z,
           "fel_nodata": np.float32(M.FEL_NODATA), "dxc": g["dxc"], "dyc": g["dyc"], "gt": np.array(gt), "geographic": np.bool_(geographic),
           "dn": np.array(dns, np.float64), "niter": np.array([M.niter_of(d, g["dxc"], g["dyc"]) for d in dns], np.int64)}
    agree = []
    with tempfile.TemporaryDirectory() as d:
        f = lambda s: os.path.join(d, s)  # noqa: E731
        T.write_raster(f("p.tif"), p, M.P_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("src.tif"), src, M.SRC_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("ad8.tif"), ad8i, -1, geotransform=gt, geographic=geographic)
        T.write_raster(f("fel.tif"), fel, M.FEL_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("z.tif"), z, M.FEL_NODATA, geotransform=gt, geographic=geographic)
        runs = [("fdc", "zfdc", ["-p", f("p.tif"), "-z", f("z.tif")], "-zfdc"),
                ("vdist", "vdist_src", ["-p", f("p.tif"), "-fel", f("fel.tif"), "-src", f("src.tif")], "-dist"),
                ("vdist", "vdist_ad8", ["-p", f("p.tif"), "-fel", f("fel.tif"), "-src", f("ad8.tif"), "-thresh", str(M.THRESH_AD8)], "-dist")]
        runs += [("slpd", f"slpd_{i}", ["-p", f("p.tif"), "-fel", f("fel.tif"), "-dn", repr(float(dn))], "-slpd") for i, dn in enumerate(dns)]
        for exe, key, args, outflag in runs:
            _, err, _ = O.run_ref(exes[exe], args + [outflag, f(key + ".tif")])
            res[key], _ = T.read_raster(f(key + ".tif"), np.float32)
            if exe == "slpd":
                i = int(key[-1])
                assert f"interations to do {int(res['niter'][i])}" in err, (key, err[-300:])
            if check_ranks:
                O.run_ref(exes[exe], args + [outflag, f(key + "3.tif")], check_ranks)
                a3, _ = T.read_raster(f(key + "3.tif"), np.float32)
                agree.append((key, bool(np.array_equal(a3.view(np.uint32), res[key].view(np.uint32)))))
    np.savez_compressed(os.path.join(OUT, f"d8last_{name}.npz"), **res)
    low = float(np.mean(res["zfdc"].view(np.uint32) != z.view(np.uint32)))
    print(name, p.shape, "niter", res["niter"].tolist(), "dn", dns, f"zfdc lowered {100 * low:.1f} %",
          "slpd valued", [f"{100 * float(np.mean(res[f'slpd_{i}'] > -1e30)):.0f} %" for i in range(3)],
          "vdist valued", f"{100 * float(np.mean(res['vdist_src'] > -1e30)):.0f} %")
    if agree:
        print(f"  {check_ranks} ranks vs 1 rank:", "; ".join(f"{k}: {'same' if a else 'DIFFERENT'}" for k, a in agree))
        assert all(a for _, a in agree), "the reference's multi-rank run differs from its 1-rank run"


if __name__ == "__main__":
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exes = {"fdc": R.build_tool(tmp, "flowdircond", ("flowdircond", "flowdirconditionmn")),
                "vdist": R.build_tool(tmp, "d8vdisttostrm", ("D8VDistToStrm", "D8VDistToStrmmn")),
                "slpd": R.build_tool(tmp, "slopeavedown", ("SlopeAveDown", "SlopeAveDownmn"))}
        for c in CASES:
            make(exes, c, check_ranks=3 if c in ("holes", "plain", "geographic") else 0)
