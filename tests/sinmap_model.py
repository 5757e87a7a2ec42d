"""SinmapSI's semantics as a serial C++ program (tests/sinmap/sinmap_restate.cpp), built at test time in three variants that bound what a conforming
evaluation of the reference's formulas may return:

    "double"   double arithmetic, -ffp-contract=off: the reference's own arithmetic (the golden maker holds it to the real tool bit for bit)
    "long"     long double arithmetic
    "fast"     double arithmetic, -ffp-contract=fast -march=native

    compile(dirpath)                     builds the three shared libraries with g++ into dirpath and returns a Restatement
    Restatement.run(variant, run)        (si, sat, code) of a run (a dict: slp, sca, scamin, scamax, cal, cal_nodata, regions, rminter, rmaxter, rhow)
    parse_calpar(text)                   the -calpar reader in Python: the table, or raises ValueError naming the line
    golden_runs(case) / patho_runs()     the runs tests/golden/sinmap_*.npz hold, as the golden maker and the tests walk them
    check(si, sat, gold)                 the rule the GPU is held to (below)

Path codes: 0 nodata, 1 not written (rmaxter == 0 and scamax == 0), 2 s == 0, 3 unstable, 4 stable, 5 region 1, 10 + k region 2 and 20 + k region 3 with
k the way f3s went: 0 bounds out of order (p = 1000), 1 a negative bound (p = 1000), 2 degenerate on y or b (f2s), 3 x1 == x2 (fa), 4 the difference of fai.

The rule: nodata, not-written and s == 0 cells, si == 10, sat == 2 and sat == 3 and the NaN pattern are exact; elsewhere sat is within one float ulp of the
golden and |si - golden| <= max(one float ulp of the golden, 8 * E_abs), E_abs being the case's largest |si| difference between the "double" variant
and either of the other two (stored with the golden; it never comes from the code under test).
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sinmap", "sinmap_restate.cpp")
GOLDEN = os.path.join(HERE, "golden")
CASES = ("fourway_mask", "geographic", "holes", "plain", "rect_dxdy")
VARIANTS = {"double": ["-ffp-contract=off"], "long": ["-DREAL=long double", "-ffp-contract=off"], "fast": ["-ffp-contract=fast", "-march=native"]}
FIELDS = ("id", "tmin", "tmax", "cmin", "cmax", "phimin", "phimax", "rhos")
SLP_NODATA = np.float32(-1.0)
NODATA, NOT_WRITTEN, FLAT, UNSTABLE, STABLE, REGION1, REGION2, REGION3 = 0, 1, 2, 3, 4, 5, 10, 20
ALL_CODES = (NODATA, NOT_WRITTEN, FLAT, UNSTABLE, STABLE, REGION1) + tuple(REGION2 + k for k in range(5)) + tuple(REGION3 + k for k in range(5))

# the -par of the goldens: the recharge bounds of the reference's own example call, g and rhow as the issue names them
RMINTER, RMAXTER, G, RHOW = 0.0009, 0.00135, 9.81, 1000.0
# four regions in SINMAP's customary ranges (T/R-style transmissivity, dimensionless cohesion 0 .. 0.25, friction angle 30 .. 45 degrees, soil density 2000),
# in vertical bands; region 7 is the degenerate-cohesion one, region 300 has the narrow friction range
CALPAR = ("id,tmin,tmax,cmin,cmax,phimin,phimax,rhos\n"
          "1,2.0,3.0,0.0,0.25,30.0,45.0,2000.0\n"
          "2,0.8,4.5,0.05,0.4,25.0,38.0,1800.0\n"
          "7,1.5,1.5,0.1,0.1,28.0,40.0,2200.0\n"
          "300,2.5,2.9,0.0,0.15,35.0,35.0,1600.0\n")
# the same table as a file with a duplicate id (the first wins), a hexadecimal id (0x12c = 300), an octal one (07) and a trailing blank line
CALPAR_VARIANT = ("region, tmin, tmax, cmin, cmax, phimin, phimax, rhos\n"
                  "1,2.0,3.0,0.0,0.25,30.0,45.0,2000.0\n"
                  "2, 0.8, 4.5, 0.05, 0.4, 25.0, 38.0, 1800.0\n"
                  "1,9.0,9.5,0.3,0.6,10.0,20.0,1200.0\n"
                  "07,1.5,1.5,0.1,0.1,28.0,40.0,2200.0\n"
                  "0x12c,2.5,2.9,0.0,0.15,35.0,35.0,1600.0 \n"
                  "\n")
BAND_IDS = (1, 2, 7, 300)
UNLISTED_ID = 99
SLOPE_SCALE = {"fourway_mask": 2.5, "geographic": 2.5, "holes": 2.5, "plain": 2.5, "rect_dxdy": 2.5}   # steep enough for every path code to occur


def parse_calpar(text):
    """{field: column} of a -calpar text (id int32, the rest float32), scanned the way "%i,%f,%f,%f,%f,%f,%f,%f" scans a line."""
    rows = []
    for lineno, line in enumerate(text.split("\n"), 1):
        if lineno == 1 or not line.strip():
            continue
        parts = [p.strip() for p in line.split(",")]
        try:
            if len(parts) < 8:
                raise ValueError
            s = parts[0].lower()
            neg = s.startswith("-")
            s = s.lstrip("+-")
            rid = int(s, 16) if s.startswith("0x") else int(s, 8) if len(s) > 1 and s.startswith("0") else int(s, 10)
            rows.append((-rid if neg else rid,) + tuple(np.float32(float(p)) for p in parts[1:8]))
        except ValueError:
            raise ValueError(f"line {lineno}") from None
    return {k: np.array([r[i] for r in rows], np.int32 if i == 0 else np.float32) for i, k in enumerate(FIELDS)}


def cal_grid(shape, seed, nodata=-32768):
    """Four vertical bands of BAND_IDS, with a sprinkle of nodata cells and of UNLISTED_ID"""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    cal = np.empty(shape, np.int16)
    for b, rid in enumerate(BAND_IDS):
        cal[:, b * nx // 4:(b + 1) * nx // 4] = rid
    r = rng.random(shape)
    cal[r < 0.01] = nodata
    cal[(r >= 0.01) & (r < 0.02)] = UNLISTED_ID
    return cal


def roads(shape, seed):
    """(scamin, scamax): zero on most cells, positive on about a fifth, a few negative (nodata) ones"""
    rng = np.random.default_rng(seed)
    on = rng.random(shape) < 0.2
    lo = np.where(on, rng.uniform(0.0, 0.02, shape), 0.0).astype(np.float32)
    hi = np.where(on, lo + rng.uniform(0.0, 0.05, shape), 0.0).astype(np.float32)
    bad = rng.random(shape) < 0.005
    lo[bad] = -1.0
    bad = rng.random(shape) < 0.005
    hi[bad] = -1.0
    return lo, hi


def _run(slp, sca, cal, calpar=CALPAR, scamin=None, scamax=None, cal_nodata=-32768, rminter=RMINTER, rmaxter=RMAXTER, rhow=RHOW, slp_nodata=SLP_NODATA):
    return {"slp": np.ascontiguousarray(slp, np.float32), "sca": np.ascontiguousarray(sca, np.float32), "cal": np.ascontiguousarray(cal, np.int16), "calpar": calpar,
            "regions": parse_calpar(calpar), "scamin": scamin, "scamax": scamax, "cal_nodata": cal_nodata, "rminter": float(np.float32(rminter)),
            "rmaxter": float(np.float32(rmaxter)), "g": G, "rhow": float(np.float32(rhow)), "slp_nodata": np.float32(slp_nodata)}


def case_inputs(name):
    """slp (scaled; nodata stays -1) and sca of case_<name>.npz"""
    g = np.load(os.path.join(GOLDEN, f"case_{name}.npz"))
    slp, sca = g["slp"], g["sca"]
    slp = np.where(slp == SLP_NODATA, SLP_NODATA, slp * np.float32(SLOPE_SCALE[name])).astype(np.float32)
    return slp, sca.astype(np.float32)


def golden_runs(name):
    """[(key, run)] of the runs sinmap_<name>.npz holds"""
    slp, sca = case_inputs(name)
    seed = 7000 + slp.shape[0] * 3 + slp.shape[1]
    cal = cal_grid(slp.shape, seed)
    lo, hi = roads(slp.shape, seed + 1)
    calpos = np.where(cal == -32768, np.int16(2), cal).astype(np.int16)   # positive cal nodata that is also a listed id: the nodata test comes first
    return [("noroads", _run(slp, sca, cal)),
            ("roads", _run(slp, sca, cal, scamin=lo, scamax=hi)),
            ("r0_noroads", _run(slp, sca, cal, rmaxter=0.0)),
            ("r0_roads", _run(slp, sca, cal, scamin=lo, scamax=hi, rmaxter=0.0)),
            ("posnd", _run(slp, sca, calpos, cal_nodata=2)),
            ("calpar_variant", _run(slp, sca, cal, calpar=CALPAR_VARIANT))]


def patho_runs():
    """[(key, run)] of sinmap_patho.npz: small rasters at their own sizes"""
    rng = np.random.default_rng(424242)
    shape = (9, 37)
    n = shape[0] * shape[1]
    slp = rng.uniform(0.05, 2.5, shape).astype(np.float32)
    sca = np.exp(rng.uniform(0.0, 9.0, shape)).astype(np.float32)
    cal = np.full(shape, 1, np.int16)
    head = "id,tmin,tmax,cmin,cmax,phimin,phimax,rhos\n"

    def special(a, vals):
        a = a.copy()
        idx = rng.choice(n, 3 * len(vals), replace=False)
        for i, v in enumerate(vals):
            a.flat[idx[3 * i:3 * i + 3]] = v
        return a

    weird = (np.nan, np.inf, -np.inf)
    runs = [("slope_zero", _run(np.where(rng.random(shape) < 0.5, 0.0, slp), sca, cal)),
            ("slope_negative", _run(-slp, sca, cal)),
            ("slp_nonfinite", _run(special(slp, weird), sca, cal)),
            ("sca_nonfinite", _run(slp, special(sca, weird), cal)),
            ("both_nonfinite", _run(special(slp, weird), special(sca, weird), cal, scamin=np.zeros(shape, np.float32), scamax=special(np.zeros(shape, np.float32), weird))),
            ("cmin_eq_cmax", _run(slp, sca, cal, calpar=head + "1,2.0,3.0,0.1,0.1,30.0,45.0,2000.0\n")),
            ("phimin_eq_phimax", _run(slp, sca, cal, calpar=head + "1,2.0,3.0,0.0,0.25,35.0,35.0,2000.0\n")),
            ("rhos_lt_rhow", _run(slp, sca, cal, calpar=head + "1,2.0,3.0,0.0,0.25,30.0,45.0,800.0\n")),
            ("x1_gt_x2", _run(slp, sca, cal, calpar=head + "1,3.0,0.5,0.0,0.25,30.0,45.0,2000.0\n")),
            ("bounds_swapped", _run(slp, sca, cal, calpar=head + "1,2.0,3.0,0.3,0.05,20.0,50.0,2000.0\n")),
            ("one_cell", _run(slp[:1, :1], sca[:1, :1], cal[:1, :1]))]
    return runs


def load_golden(name):
    """{key: {"si", "sat", "code"}}, {"E_abs", "ulp_spread"} of sinmap_<name>.npz"""
    z = np.load(os.path.join(GOLDEN, f"sinmap_{name}.npz"))
    out = {}
    for k in z.files:
        if "/" in k:
            run, what = k.split("/")
            out.setdefault(run, {})[what] = z[k]
    return out, {"E_abs": float(z["E_abs"]), "ulp_spread": float(z["ulp_spread"])}


def ulp(x):
    """one float32 ulp at |x| (of the smallest normal number below it)"""
    return np.spacing(np.maximum(np.abs(x.astype(np.float32)), np.float32(1.17549435e-38))).astype(np.float64)


def check(si, sat, gold, e_abs, where=""):
    """Holds (si, sat) to the golden {"si", "sat", "code"} under the rule of the module docstring; returns the measured largest |si - golden| outside
    the exact classes (for reports)."""
    gsi, gsat, code = gold["si"], gold["sat"], gold["code"]
    assert si.dtype == np.float32 and sat.dtype == np.float32 and si.shape == gsi.shape and sat.shape == gsat.shape, where
    assert np.array_equal(np.isnan(si), np.isnan(gsi)) and np.array_equal(np.isnan(sat), np.isnan(gsat)), f"{where}: NaN pattern"
    exact = (code == NODATA) | (code == NOT_WRITTEN) | (code == FLAT)
    assert np.array_equal(si[exact], gsi[exact]) and np.array_equal(sat[exact], gsat[exact]), f"{where}: nodata / not written / s == 0 cells"
    cap = gsi == 10.0
    assert np.array_equal(si == 10.0, cap), f"{where}: the si == 10 cap"
    for v in (2.0, 3.0):
        assert np.array_equal(sat == v, gsat == v), f"{where}: sat == {v}"
    live = ~np.isnan(gsi) & ~exact
    dsat = np.abs(sat.astype(np.float64) - gsat.astype(np.float64))
    ok = ~np.isnan(gsat) & ~exact & np.isfinite(gsat)
    assert np.all(dsat[ok] <= ulp(gsat[ok])), f"{where}: sat off by {dsat[ok].max()}"
    assert np.array_equal(sat[~ok & ~np.isnan(gsat)], gsat[~ok & ~np.isnan(gsat)]), f"{where}: infinite sat"
    fin = live & np.isfinite(gsi)
    d = np.abs(si.astype(np.float64) - gsi.astype(np.float64))
    bound = np.maximum(ulp(gsi), 8.0 * e_abs)
    bad = fin & ~(d <= bound)
    assert not bad.any(), f"{where}: {int(bad.sum())} cells, worst |si - golden| = {np.nanmax(np.where(bad, d, 0))} at code {code[bad][np.argmax(d[bad])]} (bound {bound[bad].min()})"
    assert np.array_equal(si[live & ~fin], gsi[live & ~fin]), f"{where}: infinite si"
    return float(d[fin].max()) if fin.any() else 0.0


class Restatement:
    def __init__(self, libs):
        self._libs = libs
        for lib in libs.values():
            lib.sm_run.restype = None
            lib.sm_run.argtypes = [C.c_long] + [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_double, C.c_double, C.c_float] + [C.c_void_p] * 3

    def run(self, variant, r):
        slp, sca, cal = r["slp"], r["sca"], r["cal"]
        lo = None if r["scamin"] is None else np.ascontiguousarray(r["scamin"], np.float32)
        hi = None if r["scamax"] is None else np.ascontiguousarray(r["scamax"], np.float32)
        cols = [np.ascontiguousarray(r["regions"][k], np.int32 if k == "id" else np.float32) for k in FIELDS]
        si, sat, code = np.empty(slp.shape, np.float32), np.empty(slp.shape, np.float32), np.empty(slp.shape, np.uint8)
        nd = int(np.array(r["cal_nodata"]).astype(np.int64).astype(np.int16))   # (short)cal nodata
        self._libs[variant].sm_run(slp.size, slp.ctypes.data, sca.ctypes.data, lo.ctypes.data if lo is not None else None, hi.ctypes.data if hi is not None else None,
                                   cal.ctypes.data, float(r["slp_nodata"]), nd, len(cols[0]), *[c.ctypes.data for c in cols], r["rminter"], r["rmaxter"], r["rhow"],
                                   si.ctypes.data, sat.ctypes.data, code.ctypes.data)
        return si, sat, code


def compile(dirpath):
    libs = {}
    for name, flags in VARIANTS.items():
        lib = os.path.join(str(dirpath), f"sinmap_restate_{name}.so")
        subprocess.run(["g++", "-O2", "-std=c++17", *flags, "-shared", "-fPIC", SRC, "-o", lib], check=True)
        libs[name] = C.CDLL(lib)
    return Restatement(libs)
