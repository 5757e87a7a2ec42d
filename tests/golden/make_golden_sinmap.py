"""Golden vectors for SinmapSI (src/SinmapSI.cpp): runs the REAL reference tool.  Build container only, after build() has left the reference's common
objects in oracle/_ref/obj:

    python tests/golden/make_golden_sinmap.py [--time-4096]

The reference tool is compiled into a temporary directory with make_golden_d8rev.build_tool; nothing is written under oracle/.
sinmap_<case>.npz, for the five committed cases (the runs of sinmap_model.golden_runs: slp scaled, sca, a four-region cal grid with nodata cells and an
unlisted id): si, sat and the path code of every run - without roads, with both roads, rmaxter = 0 without and with roads, a positive cal nodata, a
-calpar with a duplicate id, a hexadecimal and an octal id and a trailing blank line.  Every run is repeated on 3 ranks and the script ASSERTS that the
output equals the 1-rank output.  sinmap_patho.npz: the runs of sinmap_model.patho_runs at their own sizes, one rank.
The script asserts that the "double" restatement (tests/sinmap/sinmap_restate.cpp) equals the real tool bit for bit, NaN patterns included, that the
three restatement variants take the same path in every cell and agree on sat bit for bit and on the si == 10 cap (knife-edge cells are kept out of the
fixtures by changing seeds and scales, not by letting a test skip them), and that every path code occurs in the committed set.  Per file it stores
E_abs, the largest |si| difference between the "double" variant and either of the other two, and ulp_spread, the largest such difference in float ulps
over the cells with |si| >= 2^-5.  --time-4096 also prints the reference's own "Compute time" on a 4096 x 4096 raster tiled from `plain`.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_d8rev as R  # noqa: E402
import sinmap_model as M  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """equal bit for bit, any NaN counting as equal to any NaN at the same place"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def run(exe, d, r, ranks=1, want_stdout=False):
    f = lambda s: os.path.join(d, s)  # noqa: E731
    ny = r["slp"].shape[0]
    gt = (1000.0, 30.0, 0.0, 5000.0 + 30.0 * ny, 0.0, -30.0)
    T.write_raster(f("slp.tif"), r["slp"], float(r["slp_nodata"]), geotransform=gt)
    T.write_raster(f("sca.tif"), r["sca"], -1.0, geotransform=gt)
    T.write_raster(f("cal.tif"), r["cal"], float(r["cal_nodata"]), geotransform=gt)
    open(f("calpar.csv"), "w").write(r["calpar"])
    args = ["-slp", f("slp.tif"), "-sca", f("sca.tif"), "-calpar", f("calpar.csv"), "-cal", f("cal.tif"), "-si", f("si.tif"), "-sat", f("sat.tif"), "-par",
            repr(r["rminter"]), repr(r["rmaxter"]), repr(r["g"]), repr(r["rhow"])]
    for k in ("scamin", "scamax"):
        if r[k] is not None:
            T.write_raster(f(k + ".tif"), r[k], -1.0, geotransform=gt)
            args += ["-" + k, f(k + ".tif")]
    if len(args) + 1 <= 13:   # the flag form needs more than 12 words
        raise AssertionError("flag form too short")
    for o in ("si.tif", "sat.tif"):
        if os.path.exists(f(o)):
            os.remove(f(o))
    res = O.run_ref(exe, args, ranks)
    si, info = T.read_raster(f("si.tif"), np.float32)
    sat, info2 = T.read_raster(f("sat.tif"), np.float32)
    assert float(info["nodata"]) == -1.0 and float(info2["nodata"]) == -1.0
    return (si, sat, res[0]) if want_stdout else (si, sat)


def one(exe, restate, tmp, key, r, ranks3):
    si, sat = run(exe, tmp, r)
    if ranks3 and r["slp"].shape[0] >= 3:
        si3, sat3 = run(exe, tmp, r, ranks=3)
        assert same_bits(si, si3) and same_bits(sat, sat3), f"{key}: the 3-rank output differs from the 1-rank output"
    v = {name: restate.run(name, r) for name in M.VARIANTS}
    dsi, dsat, code = v["double"]
    assert same_bits(si, dsi) and same_bits(sat, dsat), f"{key}: the double restatement differs from the reference in {int(np.sum(bits(si) != bits(dsi)))} si cells"
    e_abs, spread = 0.0, 0.0
    for name in ("long", "fast"):
        osi, osat, ocode = v[name]
        assert np.array_equal(code, ocode), f"{key}: variant {name} takes another path in {int(np.sum(code != ocode))} cells"
        assert same_bits(dsat, osat), f"{key}: variant {name} differs in sat in {int(np.sum(bits(dsat) != bits(osat)))} cells"
        assert np.array_equal(dsi == 10.0, osi == 10.0), f"{key}: variant {name} differs on the cap"
        fin = np.isfinite(dsi) & np.isfinite(osi)
        d = np.abs(dsi.astype(np.float64) - osi.astype(np.float64))
        if fin.any():
            e_abs = max(e_abs, float(d[fin].max()))
        big = fin & (np.abs(dsi) >= 2.0 ** -5)
        if big.any():
            spread = max(spread, float((d[big] / M.ulp(dsi[big])).max()))
    return {"si": si, "sat": sat, "code": code}, e_abs, spread


def save(name, results, e_abs, spread):
    flat = {f"{k}/{w}": a for k, res in results.items() for w, a in res.items()}
    np.savez_compressed(os.path.join(OUT, f"sinmap_{name}.npz"), E_abs=np.float64(e_abs), ulp_spread=np.float64(spread), **flat)


if __name__ == "__main__":
    O.build()
    seen = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_tool(tmp, "sinmapsi", ("SinmapSI", "SinmapSImn"))
        restate = M.compile(tmp)
        for c in M.CASES + ("patho",):
            results, e_abs, spread = {}, 0.0, 0.0
            for key, r in (M.patho_runs() if c == "patho" else M.golden_runs(c)):
                results[key], e, s = one(exe, restate, tmp, f"{c} {key}", r, ranks3=c != "patho")
                e_abs, spread = max(e_abs, e), max(spread, s)
                codes, counts = np.unique(results[key]["code"], return_counts=True)
                for k, n in zip(codes.tolist(), counts.tolist()):
                    seen[k] = seen.get(k, 0) + n
                print(c, key, r["slp"].shape, dict(zip(codes.tolist(), counts.tolist())))
            if c != "patho":
                assert not (results["r0_noroads"]["code"] > M.NOT_WRITTEN).any() and np.all(results["r0_noroads"]["si"] == -1.0)
                w = results["r0_roads"]["code"] > M.NOT_WRITTEN
                assert w.any() and np.all(M.golden_runs(c)[3][1]["scamax"][w] != 0)
            save(c, results, e_abs, spread)
            print(c, "E_abs", e_abs, "ulp spread", spread)
        missing = [k for k in M.ALL_CODES if k not in seen]
        assert not missing, f"path codes that do not occur in the committed set: {missing}"
        print("cells per path code:", dict(sorted(seen.items())))
        if "--time-4096" in sys.argv:
            r = dict(M.golden_runs("plain")[0][1])
            reps = (4096 // r["slp"].shape[0] + 1, 4096 // r["slp"].shape[1] + 1)
            for k in ("slp", "sca", "cal"):
                r[k] = np.ascontiguousarray(np.tile(r[k], reps)[:4096, :4096])
            out = run(exe, tmp, r, want_stdout=True)[2]
            print("reference at 4096 x 4096, 1 rank:", [line for line in out.splitlines() if "ompute time" in line])
