"""The five terrain-index tools as a serial C program (tests/indices/indices_restate.c), built at test time, and the runs the goldens hold.

    compile(dirpath)              builds the shared library with gcc (-ffp-contract=off) into dirpath and returns a Restatement
    Restatement.twi / sar / sa / lengtharea / setregion     the tools on numpy rasters; the log / pow tools also return each cell's margin
    crop_runs(case)               [(key, tool, run)] of a committed case cropped to at most 96 x 128: every tool, every parameter set
    hand_runs()                   [(key, tool, run)] of the hand-built rasters (tests/golden/indices_hand.npz)
    all_runs(name)                either of the two by fixture name
    load_golden(name)             {key: array} and the stored statistics of tests/golden/indices_<name>.npz

The three comparisons (the contract is in DESIGN.md, "Terrain indices"):
  1. the GPU against the restatement: bit for bit, every cell of every tool - the restatement rounds logl / powl once to float, the target the library
     is held to.  NaN cells: a NaN at the same places (the sign and payload of a NaN an operation makes differ between x86 and the GPU);
  2. the restatement against the real tool (the goldens): SlopeAreaRatio, SetRegion and every nodata / not-written pattern exact, TWI within 1 float ulp,
     SlopeArea within 6 ulp, at most 1 % of a fixture's cells different at all;
  3. LengthArea against the real tool: exact - the generator keeps cells whose float(ad8) lies within 2 ulp of the threshold out of the fixtures, except
     where the threshold is exact in any libm (y == 1; plen in {0, 1} with a power-of-two M), where it plants equalities.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "indices", "indices_restate.c")
GOLDEN = os.path.join(HERE, "golden")
CASES = ("plain", "holes", "geographic")
FIXTURES = CASES + ("hand",)
NODATA_F = np.float32(-1.0)          # slp, sca, plen and the three float outputs
P_NODATA = np.int16(-32768)
MISSINGLONG = np.int32(-2147483647)
SS_NOT_WRITTEN = np.int16(-32768)
MARGIN_MIN = 2.0 ** -40
SA_PARS = {"default": (2.0, 1.0), "negexp": (1.5, -0.75), "zeroexp": (0.0, 1.5)}
LA_PARS = {"default": (0.03, 1.3), "half_one": (0.5, 1.0)}
TWI_ULP, SA_ULP, DIFF_SHARE_CAP = 1, 6, 0.01
# Crops of at most 96 x 128 and slope scales (tests/sinmap_model.py scales the committed slopes by 2.5) under which no cell of any run lies within 2^-40 of a
# rounding boundary: the committed slopes have short mantissas, whose squares are exact ties by the dozen at 2.5, and row 75 of `geographic` holds a plen
# whose power 1.3 is a near-tie.  tests/golden/make_golden_indices.py asserts it.
CROP = {"plain": (96, 128), "holes": (96, 100), "geographic": (75, 110)}
SLOPE_SCALE = {"plain": 2.05, "holes": 2.55, "geographic": 2.5}


def same_bits(a, b):
    """equal bit for bit, a NaN counting as equal to any NaN at the same place"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def ulp_distance(a, b):
    """the distance of two float32 arrays in units in the last place (the floats ordered as integers); 0 where both are NaN, a huge number where one is"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(b))
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na & nb, 0, np.where(na | nb, 2 ** 40, d))


class Restatement:
    def __init__(self, lib):
        P, F, L = C.c_void_p, C.c_float, C.c_long
        lib.ix_twi.argtypes = [L, P, P, F, F, P, P]
        lib.ix_sar.argtypes = [L, P, P, F, P]
        lib.ix_sa.argtypes = [L, P, P, F, F, P, P, P, P]
        lib.ix_lengtharea.argtypes = [L, P, P, F, F, P, P, P, P, P]
        lib.ix_setregion.argtypes = [C.c_int, C.c_int, P, P, C.c_int16, C.c_int32, C.c_int32, P]
        for f in (lib.ix_twi, lib.ix_sar, lib.ix_sa, lib.ix_lengtharea, lib.ix_setregion):
            f.restype = None
        self._lib = lib

    @staticmethod
    def _f(a):
        return np.ascontiguousarray(a, np.float32)

    def twi(self, slp, sca, slp_nodata=NODATA_F, sca_nodata=NODATA_F):
        slp, sca = self._f(slp), self._f(sca)
        out, margin = np.empty(slp.shape, np.float32), np.empty(slp.shape, np.float64)
        self._lib.ix_twi(slp.size, slp.ctypes.data, sca.ctypes.data, float(slp_nodata), float(sca_nodata), out.ctypes.data, margin.ctypes.data)
        return out, margin

    def sar(self, slp, sca, sca_nodata=NODATA_F):
        slp, sca = self._f(slp), self._f(sca)
        out = np.empty(slp.shape, np.float32)
        self._lib.ix_sar(slp.size, slp.ctypes.data, sca.ctypes.data, float(sca_nodata), out.ctypes.data)
        return out

    def sa(self, slp, sca, m, n):
        """sa, margin, the two factors"""
        slp, sca = self._f(slp), self._f(sca)
        out, margin = np.empty(slp.shape, np.float32), np.empty(slp.shape, np.float64)
        f0, f1 = np.empty(slp.shape, np.float32), np.empty(slp.shape, np.float32)
        self._lib.ix_sa(slp.size, slp.ctypes.data, sca.ctypes.data, float(np.float32(m)), float(np.float32(n)), out.ctypes.data, margin.ctypes.data, f0.ctypes.data,
                        f1.ctypes.data)
        return out, margin, f0, f1

    def lengtharea(self, plen, ad8, M, y):
        """ss, margin, plen^y, the threshold, ad8 as int32"""
        plen, ad8 = self._f(plen), self._f(ad8)
        out, margin = np.empty(plen.shape, np.int16), np.empty(plen.shape, np.float64)
        fac, thr, ad8i = np.empty(plen.shape, np.float32), np.empty(plen.shape, np.float32), np.empty(plen.shape, np.int32)
        self._lib.ix_lengtharea(plen.size, plen.ctypes.data, ad8.ctypes.data, float(np.float32(M)), float(np.float32(y)), out.ctypes.data, margin.ctypes.data,
                                fac.ctypes.data, thr.ctypes.data, ad8i.ctypes.data)
        return out, margin, fac, thr, ad8i

    def setregion(self, p, gw, region_id=1, p_nodata=P_NODATA, gw_nodata=MISSINGLONG):
        p, gw = np.ascontiguousarray(p, np.int16), np.ascontiguousarray(gw, np.int32)
        out = np.empty(p.shape, np.int32)
        self._lib.ix_setregion(p.shape[1], p.shape[0], p.ctypes.data, gw.ctypes.data, int(p_nodata), int(gw_nodata), int(region_id), out.ctypes.data)
        return out

    def run(self, tool, r):
        """the output of a run (below) alone"""
        if tool == "twi":
            return self.twi(r["slp"], r["sca"])[0]
        if tool == "sar":
            return self.sar(r["slp"], r["sca"])
        if tool == "sa":
            return self.sa(r["slp"], r["sca"], *r["par"])[0]
        if tool == "la":
            return self.lengtharea(r["plen"], r["ad8"], *r["par"])[0]
        return self.setregion(r["p"], r["gw"], r["id"])


def compile(dirpath):
    lib = os.path.join(str(dirpath), "indices_restate.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", lib, "-lm"], check=True)
    return Restatement(C.CDLL(lib))


def case_inputs(name):
    """The rasters of a committed case, cropped to CROP[name]: slp (scaled; nodata stays -1) and sca of case_<name>.npz, plen of its gridnet golden, the integer
    ad8, p and gw of its gagewatershed golden (d8rev_<name>.npz; gw has nodata holes, p a few zeros and out-of-range values), and the weighted ad8."""
    g = np.load(os.path.join(GOLDEN, f"case_{name}.npz"))
    n = np.load(os.path.join(GOLDEN, f"case_{name}_gridnet.npz"))
    d = np.load(os.path.join(GOLDEN, f"d8rev_{name}.npz"))
    c = lambda a: np.ascontiguousarray(a[:CROP[name][0], :CROP[name][1]])  # noqa: E731
    slp = np.where(g["slp"] == NODATA_F, NODATA_F, g["slp"] * np.float32(SLOPE_SCALE[name])).astype(np.float32)
    return {"slp": c(slp), "sca": c(g["sca"].astype(np.float32)), "plen": c(n["plen"].astype(np.float32)), "ad8": c(d["ad8"].astype(np.float32)),
            "ad8_w": c(g["ad8_w"].astype(np.float32)), "p": c(d["p"].astype(np.int16)), "gw": c(d["gw"].astype(np.int32))}


def crop_runs(name):
    i = case_inputs(name)
    runs = [("twi", "twi", {"slp": i["slp"], "sca": i["sca"]}), ("sar", "sar", {"slp": i["slp"], "sca": i["sca"]})]
    runs += [(f"sa_{k}", "sa", {"slp": i["slp"], "sca": i["sca"], "par": par}) for k, par in SA_PARS.items()]
    runs += [(f"la_{k}", "la", {"plen": i["plen"], "ad8": i["ad8"], "par": par}) for k, par in LA_PARS.items()]
    runs += [("setregion", "setregion", {"p": i["p"], "gw": i["gw"], "id": 1}), ("setregion_id7", "setregion", {"p": i["p"], "gw": i["gw"], "id": 7})]
    return runs


def special_terrain():
    """slp, sca (3 x 8): zeros, nodata on either side, values within and just outside MINEPS of the nodata value, NaN and inf, a quotient that overflows and
    a subnormal one.  The negative zeros stand in the middle row: after its loop the reference adds a (zero) border to the first and the last row
    of every rank's partition, which turns a -0.0 result there into +0.0 - an artefact of the rank count that the library does not reproduce."""
    nan, inf = np.nan, np.inf
    slp = np.array([[0.0, 0.5, 0.0, -1.0, 0.25, nan, 0.5, inf],
                    [2.0, 1.0, 3.0, 1e-20, 1e20, -0.0, 0.5, -inf],
                    [inf, 1e-3, 1e10, 0.5, 0.5, -0.999995, -0.99998, 1.0]], np.float32)
    sca = np.array([[30.0, 0.0, 0.0, 30.0, -1.0, 30.0, nan, 30.0],
                    [8.0, 2.0, 27.0, 1e20, 1e-20, 30.0, -0.0, 30.0],
                    [inf, 3e38, 1e-30, -0.999995, -0.99998, 30.0, 30.0, 1.0]], np.float32)
    return slp, sca


def hole_blocks():
    """p, gw (5 x 60): twelve 5 x 5 blocks of holes (nodata in p and in gw) with one live cell next to the block's centre: blocks 0..7 the neighbour k = 1..8
    draining into the centre, 8 a neighbour draining away, 9 one with p == 0, 10 one with p == -3 east of the centre (|p - 1| == 4, held off by p > 0 alone),
    11 one with data in gw and none in p"""
    dx = (0, 1, 1, 0, -1, -1, -1, 0, 1)
    dy = (0, 0, -1, -1, -1, 0, 1, 1, 1)
    p = np.full((5, 60), P_NODATA, np.int16)
    gw = np.full((5, 60), MISSINGLONG, np.int32)
    for b in range(12):
        k = b + 1 if b < 8 else 1
        y, x = 2 + dy[k], 5 * b + 2 + dx[k]
        if b < 8:
            p[y, x] = k + 4 if k <= 4 else k - 4
        elif b == 8:
            p[y, x] = 1          # the east neighbour flows east
        elif b == 9:
            p[y, x] = 0
        elif b == 10:
            p[y, x] = -3
        else:
            gw[y, x] = 42
    return p, gw


def edge_holes():
    """p, gw (6 x 7): holes all around the edge, corners included, and directions 1..8 in turn inside"""
    p = np.full((6, 7), P_NODATA, np.int16)
    gw = np.full((6, 7), MISSINGLONG, np.int32)
    k = 0
    for y in range(1, 5):
        for x in range(1, 6):
            p[y, x] = k % 8 + 1
            gw[y, x] = 3 if (x + y) % 3 else MISSINGLONG
            k += 3
    return p, gw


def planted_lengtharea():
    """plen, ad8 (2 x 8) for -par 0.5 1: ad8 on the threshold (six cells), one below, one above, a negative and a NaN length;
    plen, ad8 (1 x 6) for -par 2 1.3: plen in {0, 1}, ad8 on the threshold, below and above"""
    nan = np.nan
    a = (np.array([[2.0, 4.0, 10.0, 256.0, 0.0, 6.0, 6.0, 6.0], [-1.0, nan, -0.5, 3.0, 7.0, 1.0, 0.5, 100.0]], np.float32),
         np.array([[1.0, 2.0, 5.0, 128.0, 0.0, 3.0, 2.0, 4.0], [5.0, 5.0, 5.0, 2.0, 3.0, 0.0, 1.0, 50.0]], np.float32))
    b = (np.array([[0.0, 1.0, 1.0, 1.0, 0.0, 0.0]], np.float32), np.array([[0.0, 2.0, 1.0, 3.0, -1.0, 1.0]], np.float32))
    return a, b


def hand_runs():
    rng = np.random.default_rng(20260)
    slp = rng.uniform(0.01, 2.0, (5, 7)).astype(np.float32)
    sca = np.exp(rng.uniform(0.0, 9.0, (5, 7))).astype(np.float32)
    runs = []
    for key, sl in (("one_cell", np.s_[:1, :1]), ("one_row", np.s_[:1, :]), ("one_column", np.s_[:, :1])):
        s, a = np.ascontiguousarray(slp[sl]), np.ascontiguousarray(sca[sl])
        runs += [(f"{key}_twi", "twi", {"slp": s, "sca": a}), (f"{key}_sar", "sar", {"slp": s, "sca": a}), (f"{key}_sa", "sa", {"slp": s, "sca": a, "par": SA_PARS["default"]})]
        pl = (a * np.float32(3.0)).astype(np.float32)
        ad = np.floor(a).astype(np.float32)
        runs.append((f"{key}_la", "la", {"plen": pl, "ad8": ad, "par": LA_PARS["default"]}))
    s, a = special_terrain()
    runs += [("special_twi", "twi", {"slp": s, "sca": a}), ("special_sar", "sar", {"slp": s, "sca": a})]
    runs += [(f"special_sa_{k}", "sa", {"slp": s, "sca": a, "par": par}) for k, par in SA_PARS.items()]
    (pl, ad), (pl2, ad2) = planted_lengtharea()
    runs += [("planted_la_half_one", "la", {"plen": pl, "ad8": ad, "par": LA_PARS["half_one"], "planted": True}),
             ("planted_la_two", "la", {"plen": pl2, "ad8": ad2, "par": (2.0, 1.3), "planted": True})]
    p, gw = hole_blocks()
    runs.append(("hole_blocks", "setregion", {"p": p, "gw": gw, "id": 1}))
    p, gw = edge_holes()
    runs.append(("edge_holes", "setregion", {"p": p, "gw": gw, "id": 5}))
    for key, sl in (("one_cell", np.s_[:1, :1]), ("one_row", np.s_[:1, :]), ("one_column", np.s_[:, 1:2])):
        runs.append((f"{key}_setregion", "setregion", {"p": np.ascontiguousarray(p[sl]), "gw": np.ascontiguousarray(gw[sl]), "id": 2}))
    return runs


def fractional_run():
    """LengthArea on a weighted (fractional) ad8 with halves, negative values and a NaN planted: held against the restatement only"""
    i = case_inputs("plain")
    ad8 = i["ad8_w"].copy()
    ad8[3, :8] = (2.5, 3.5, -0.5, -1.5, 0.5, np.nan, 1e10, -1e10)
    return ("la_fractional", "la", {"plen": i["plen"], "ad8": ad8, "par": LA_PARS["default"]})


def all_runs(name):
    return hand_runs() if name == "hand" else crop_runs(name)


def load_golden(name):
    """{key: the real tool's output}, {key: {"max_ulp", "diff_share"}} for the log / pow runs, the glibc version of the host that made them"""
    z = np.load(os.path.join(GOLDEN, f"indices_{name}.npz"))
    out, stats = {}, {}
    for k in z.files:
        if k.startswith("out/"):
            out[k[4:]] = z[k]
        elif k.startswith("stat/"):
            key, what = k[5:].rsplit("/", 1)
            stats.setdefault(key, {})[what] = float(z[k])
    return out, stats, str(z["glibc"])
