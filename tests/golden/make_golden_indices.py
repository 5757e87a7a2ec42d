"""Golden vectors for TWI, SlopeArea, SlopeAreaRatio, LengthArea and SetRegion: runs the REAL reference tools.  Build container only, after build() has left
the reference's common objects in oracle/_ref/obj:

    python tests/golden/make_golden_indices.py

The five tools are compiled into a temporary directory with make_golden_d8rev.build_tool; nothing is written under oracle/.  indices_<case>.npz holds, for
the runs of indices_model.crop_runs(case) and indices_hand.npz for those of indices_model.hand_runs(), the real tool's output raster ("out/<run>"), and for
the log / pow runs the largest distance in float ulps between the tool and the restatement and the share of cells that differ at all
("stat/<run>/max_ulp", "stat/<run>/diff_share"), with the glibc version of this host ("glibc").  Every run with six rows or more is repeated on 3 ranks
and the script ASSERTS that the output equals the 1-rank output (a rank that owns a single row adds a border buffer nobody wrote into that row in the
four float / short tools - addBorders() after the loop - and writes garbage there: the 1-rank output is the tool's meaning).  It asserts the contract of tests/indices_model.py on every committed cell:

  * no cell's log or pow value lies within 2^-40 (relative) of a float rounding boundary, and no finite pow factor or product within 4 ulp of overflow
    or of the edge of the subnormal range;
  * SlopeAreaRatio, SetRegion and the nodata / not-written patterns of all five equal the restatement exactly; TWI within 1 ulp, SlopeArea within 6,
    and the real tool's share of differing cells under the 1 % cap;
  * LengthArea equals the restatement exactly, and no cell's float(ad8) lies within 2 ulp of its threshold, except in runs whose threshold is exact in any
    libm (y == 1, or the planted plen in {0, 1} with a power-of-two M); those hold at least six cells with ad8 ON the threshold.

A tripped margin or range assertion is met by changing a crop, a scale or a seed in tests/indices_model.py, never by letting a test skip cells.
"""
import os
import platform
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import indices_model as M  # noqa: E402
import make_golden_d8rev as R  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
TOOLS = {"twi": ("twi", ("TWI", "TWImn")), "sa": ("slopearea", ("SlopeArea", "SlopeAreamn")), "sar": ("slopearearatio", ("SlopeAreaRatio", "SlopeAreaRatiomn")),
         "la": ("lengtharea", ("LengthArea", "LengthAreamn")), "setregion": ("setregion", ("SetRegion", "SetRegionmn"))}
FLT_MAX, FLT_MIN, EPS = float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny), 2.0 ** -23


def run_tool(exes, d, tool, r, ranks):
    f = lambda s: os.path.join(d, s)  # noqa: E731
    first = r["p" if tool == "setregion" else "plen" if tool == "la" else "slp"]
    gt = (1000.0, 30.0, 0.0, 5000.0 + 30.0 * first.shape[0], 0.0, -30.0)
    out = f("out.tif")
    if os.path.exists(out):
        os.remove(out)
    if tool in ("twi", "sa", "sar"):
        T.write_raster(f("slp.tif"), r["slp"], float(M.NODATA_F), geotransform=gt)
        T.write_raster(f("sca.tif"), r["sca"], float(M.NODATA_F), geotransform=gt)
        args = ["-slp", f("slp.tif"), "-sca", f("sca.tif"), "-" + tool, out]
        if tool == "sa":
            args += ["-par", repr(float(r["par"][0])), repr(float(r["par"][1]))]
        dtype, nodata = np.float32, -1.0
    elif tool == "la":
        T.write_raster(f("plen.tif"), r["plen"], float(M.NODATA_F), geotransform=gt)
        assert np.array_equal(r["ad8"], np.round(r["ad8"])), "the real tool is given integer-valued ad8 only"
        T.write_raster(f("ad8.tif"), r["ad8"].astype(np.int32), -1, geotransform=gt)
        args = ["-plen", f("plen.tif"), "-ad8", f("ad8.tif"), "-ss", out, "-par", repr(float(r["par"][0])), repr(float(r["par"][1]))]
        dtype, nodata = np.int16, -32768.0
    else:
        T.write_raster(f("p.tif"), r["p"], int(M.P_NODATA), geotransform=gt)
        T.write_raster(f("gw.tif"), r["gw"], int(M.MISSINGLONG), geotransform=gt)
        args = ["-p", f("p.tif"), "-gw", f("gw.tif"), "-out", out, "-id", str(r["id"])]
        dtype, nodata = np.int32, float(M.MISSINGLONG)
    O.run_ref(exes[tool], args, ranks)
    a, info = T.read_raster(out, dtype)
    assert float(info["nodata"]) == nodata and a.dtype == dtype, (tool, info["nodata"], a.dtype)
    return a


def near_range_edge(v):
    """finite, non-zero values within 4 ulp of overflow or of the edge of the subnormal range"""
    a = np.abs(v.astype(np.float64))
    live = np.isfinite(a) & (a != 0)
    return live & ((a > FLT_MAX * (1 - 4 * EPS)) | ((a > FLT_MIN * (1 - 4 * EPS)) & (a < FLT_MIN * (1 + 4 * EPS))))


def near_threshold(plen, ss, thr, ad8i):
    """evaluated cells whose float(ad8) lies within 2 ulp of a threshold that a libm within its bound could move: plen^y is exact for plen in {0, 1}"""
    d = M.ulp_distance(ad8i.astype(np.float32), thr)
    return (ss != M.SS_NOT_WRITTEN) & np.isfinite(thr) & (d <= 2) & (plen != 0) & (plen != 1)


def check_run(restate, key, tool, r, got):
    """the contract on one run; returns the statistics that go into the file"""
    stat = {}
    if tool == "sar":
        assert M.same_bits(got, restate.sar(r["slp"], r["sca"])), f"{key}: SlopeAreaRatio differs from the restatement"
    elif tool == "setregion":
        assert np.array_equal(got, restate.setregion(r["p"], r["gw"], r["id"])), f"{key}: SetRegion differs from the restatement"
    elif tool == "la":
        ss, margin, fac, thr, ad8i = restate.lengtharea(r["plen"], r["ad8"], *r["par"])
        assert np.array_equal(got, ss), f"{key}: LengthArea differs from the restatement in {int(np.sum(got != ss))} cells"
        live = ss != M.SS_NOT_WRITTEN
        assert margin[live].min(initial=1.0) >= M.MARGIN_MIN, f"{key}: margin {margin[live].min()}"
        assert not near_range_edge(fac).any() and not near_range_edge(thr).any(), f"{key}: a factor or threshold at the edge of the float range"
        on = live & (ad8i.astype(np.float32) == thr)
        if r["par"][1] == 1.0 or r.get("planted"):
            stat["on_threshold"] = float(on.sum())
        else:
            assert not near_threshold(r["plen"], ss, thr, ad8i).any(), f"{key}: cells within 2 ulp of the threshold"
    else:
        if tool == "twi":
            want, margin = restate.twi(r["slp"], r["sca"])
            bound = M.TWI_ULP
        else:
            want, margin, f0, f1 = restate.sa(r["slp"], r["sca"], *r["par"])
            bound = M.SA_ULP
            assert not near_range_edge(f0).any() and not near_range_edge(f1).any() and not near_range_edge(want).any(), f"{key}: a factor or product at the edge of the float range"
        assert margin.min() >= M.MARGIN_MIN, f"{key}: margin {margin.min()} in {int((margin < M.MARGIN_MIN).sum())} cells"
        assert np.array_equal(got == -1.0, want == -1.0) and np.array_equal(np.isnan(got), np.isnan(want)), f"{key}: nodata or NaN pattern"
        d = M.ulp_distance(got, want)
        stat["max_ulp"], stat["diff_share"] = float(d.max()), float((d != 0).mean())
        assert d.max() <= bound, f"{key}: {d.max()} ulp from the restatement"
        assert stat["diff_share"] <= M.DIFF_SHARE_CAP, f"{key}: {stat['diff_share']} of the cells differ"
    return stat


if __name__ == "__main__":
    O.build()
    glibc = " ".join(platform.libc_ver())
    with tempfile.TemporaryDirectory() as tmp:
        exes = {tool: R.build_tool(tmp, name, srcs) for tool, (name, srcs) in TOOLS.items()}
        restate = M.compile(tmp)
        planted = 0
        for name in M.FIXTURES:
            data = {"glibc": np.array(glibc)}
            for key, tool, r in M.all_runs(name):
                got = run_tool(exes, tmp, tool, r, 1)
                if got.shape[0] >= 6:   # two rows per rank at least: see the module docstring
                    assert M.same_bits(got, run_tool(exes, tmp, tool, r, 3)), f"{name} {key}: the 3-rank output differs from the 1-rank output"
                stat = check_run(restate, f"{name} {key}", tool, r, got)
                planted += int(stat.get("on_threshold", 0))
                data[f"out/{key}"] = got
                for k, v in stat.items():
                    data[f"stat/{key}/{k}"] = np.float64(v)
                print(name, key, got.shape, stat)
            np.savez_compressed(os.path.join(OUT, f"indices_{name}.npz"), **data)
        assert planted >= 6, f"only {planted} cells with ad8 on the threshold"
        key, tool, r = M.fractional_run()   # no golden: the real tool is not run on a fractional ad8; the margins still hold
        ss, margin, fac, thr, ad8i = restate.lengtharea(r["plen"], r["ad8"], *r["par"])
        assert margin[ss != M.SS_NOT_WRITTEN].min() >= M.MARGIN_MIN
        assert not near_threshold(r["plen"], ss, thr, ad8i).any(), "fractional run: cells within 2 ulp of the threshold"
        print("glibc:", glibc, "cells on a threshold:", planted)
