"""Golden vectors for DropAnalysis (src/DropAnalysis.cpp): runs the REAL reference tool on the committed cases.  Build container only, after build()
has left the reference's common objects in oracle/_ref/obj:

    python tests/golden/make_golden_dropan.py [--patho-only]      (--patho-only: dropan_patho.npz alone, the five case files are left as they are)

The reference tool is compiled into a temporary directory with make_golden_d8rev.build_tool; nothing is written under oracle/.  The inputs are those of
case_<case>.npz: p, fel, and ad8 both as the area raster and as ssa (any raster that increases downstream serves).  dropan_<case>.npz holds
  * cols, rows: the outlets of make_golden_d8rev.outlets - with one change: its outlet "five steps downstream" lands on the raster's nodata ring in every
    case, where the reference indexes outside its offset table (the product refuses such an outlet); it is moved one step back, to the neighbour with the
    largest ad8 that drains into it.  That outlet is then the only terminal one (its downstream neighbour has ssa nodata) and makes the total area.
    One outlet is a repeat and one lies off the raster.
  * par = (min, max, nthresh) of -par; for each step type s (0 log, 1 arithmetic): table_s, console_s, the bytes of the table file and of stdout on one
    rank, and noise_s (5 values: MeanDFirstOrd, MeanDHighOrd, StdDevFirstOrd, StdDevHighOrd, T) - the largest difference, over the rows, between the
    reference's table and the table made from CORRECTLY ROUNDED sums (math.fsum of the drop lists of tests/dropan/dropan_restate.cpp, rounded to float):
    the reference's own rounding noise, from adding in float in queue order.
  * for `plain` and `geographic`: table3_s from 3 ranks.  Whether it equals the 1-rank table is printed, not asserted: the float sums are added in rank order.
The parameters are chosen so that every run writes at least six rows, `plain`, `holes`, `rect_dxdy` and `fourway_mask` (log) have an optimum that is not the
first row, and exactly one run (`fourway_mask`, arithmetic) has none.  The script asserts that the restatement's table equals the reference's byte for byte
and that no |t| of the reference lies within 0.01 of 2 (console lines, every threshold): a condition on the inputs - if it fails, pick other parameters.
The files are named dropan_*.npz, not case_*.npz: conftest.golden_cases() takes every case_*.npz as a case.

dropan_patho.npz: the reference on the rasters of tests/pathological.py, one rank, both step types.  The inputs are not stored: dropan_strips.patho_case
derives fel, p and ad8 from the generator's raster with the CPU oracle (30 x 30 cells, ssa = ad8), and the tests derive them again.  Per case <name> the
file holds cols_<name>, rows_<name>, par_<name> and, per step type s, table_<name>_s and console_<name>_s.  A case the reference does not finish on (it is
given PATHO_TIMEOUT seconds) is left out if no cell of it has a direction 1..8; any other failure stops the script.  Here too the restatement's table must
equal the reference's byte for byte; rows, optimum and min ||t| - 2| are printed per run, and at the end the cases that were left out.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import dropan_model as M  # noqa: E402
import make_golden_d8rev as R  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
PAR = {"plain": (1, 30, 10), "holes": (3, 60, 10), "rect_dxdy": (2, 40, 14), "geographic": (1, 30, 10), "fourway_mask": (2, 40, 14)}
NO_OPTIMUM = ("fourway_mask", 1)
PATHO_TIMEOUT = 120


def as_bytes(b):
    return np.frombuffer(b, np.uint8).copy()


def outlets(p, ad8):
    """make_golden_d8rev.outlets with the outlet on a cell without a direction moved one step back up the flow path."""
    ny, nx = p.shape
    ad8i = np.where(ad8 < -0.5, -1, np.rint(ad8)).astype(np.int32)
    cols, rows, _ = R.outlets(p, ad8i)
    for i, (c, r) in enumerate(zip(cols.tolist(), rows.tolist())):
        if 0 <= c < nx and 0 <= r < ny and not 0 <= p[r, c] <= 8:
            feeds = [(float(ad8[r + R.DY_[k], c + R.DX_[k]]), c + R.DX_[k], r + R.DY_[k]) for k in range(1, 9)
                     if 0 <= c + R.DX_[k] < nx and 0 <= r + R.DY_[k] < ny and 1 <= p[r + R.DY_[k], c + R.DX_[k]] <= 8
                     and abs(int(p[r + R.DY_[k], c + R.DX_[k]]) - k) == 4]
            _, cols[i], rows[i] = max(feeds)
    return cols, rows


def make(exe, restate, name, ranks3=False):
    g = np.load(os.path.join(OUT, f"case_{name}.npz"))
    p, fel, ad8 = g["p"], g["fel"], g["ad8"]
    ny, nx = p.shape
    dx, dy, geographic = float(g["dx"]), float(g["dy"]), bool(g["geographic"])
    gt = (-111.9, dx, 0.0, 41.9, 0.0, -dy) if geographic else (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)
    cols, rows = outlets(p, ad8)
    par = PAR[name]
    res = {"cols": cols, "rows": rows, "par": np.array(par, np.float64)}
    with tempfile.TemporaryDirectory() as d:
        f = lambda s: os.path.join(d, s)  # noqa: E731
        T.write_raster(f("p.tif"), p, M.P_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("fel.tif"), fel, float(T.FEL_NODATA), geotransform=gt, geographic=geographic)
        T.write_raster(f("ad8.tif"), ad8, -1.0, geotransform=gt, geographic=geographic)
        with open(f("outlets.txt"), "w") as fo:
            for i, (c, r) in enumerate(zip(cols, rows)):
                fo.write(f"{float(gt[0] + (c + 0.5) * dx)!r} {float(gt[3] - (r + 0.5) * dy)!r} {i + 1}\n")
        for st in (0, 1):
            args = ["-ad8", f("ad8.tif"), "-p", f("p.tif"), "-fel", f("fel.tif"), "-ssa", f("ad8.tif"), "-o", f("outlets.txt"), "-par", par[0], par[1], par[2], st]
            stdout, _, _ = O.run_ref(exe, args + ["-drp", f(f"drp{st}.txt")])
            table = open(f(f"drp{st}.txt"), "rb").read()
            res[f"table_{st}"], res[f"console_{st}"] = as_bytes(table), as_bytes(stdout.encode())
            # the restatement is the reference on one rank ...
            _, info = T.read_raster(f("ad8.tif"))
            mine = restate.run(ad8, p, fel, ad8, cols, rows, info["dxc"], info["dyc"], par[0], par[1], par[2], st)
            assert mine["table"] == table, f"{name} steptype {st}: the restatement's table differs from the reference's\n{mine['table'].decode()}\n{table.decode()}"
            # ... so its drop lists are the reference's: the table of the correctly rounded sums shows the reference's rounding noise
            exact = np.array([np.array(M.sums_from_drops(q["drops1"], q["drops2"])).astype(np.float32) for q in mine["per"]])
            tab_exact, _, _ = restate.table(mine["thresh"], [q["n1"] for q in mine["per"]], [q["n2"] for q in mine["per"]], exact, [q["length"] for q in mine["per"]],
                                            mine["total_area"])
            r_ref, opt = M.parse_table(table)
            r_exact, _ = M.parse_table(tab_exact)
            assert r_ref.shape == r_exact.shape and np.array_equal(r_ref[:, :4], r_exact[:, :4])
            res[f"noise_{st}"] = np.max(np.abs(r_ref[:, 4:] - r_exact[:, 4:]), axis=0)
            ts = M.console_t(stdout.encode())
            near = float(np.min(np.abs(np.abs(ts) - 2.0)))
            assert near > 0.01, f"{name} steptype {st}: a |t| within 0.01 of 2 ({near}): pick other parameters"
            assert len(r_ref) >= 6, f"{name} steptype {st}: {len(r_ref)} rows"
            has_opt = bool(np.any(np.abs(ts) < 2.0))
            assert has_opt == ((name, st) != NO_OPTIMUM), f"{name} steptype {st}: optimum {'found' if has_opt else 'missing'}"
            print(name, p.shape, "steptype", st, "rows", len(r_ref), "optimum", opt if has_opt else None, "first row", float(r_ref[0, 0]), "min ||t| - 2|", round(near, 4), "noise",
                  res[f"noise_{st}"])
            if ranks3:
                O.run_ref(exe, args + ["-drp", f(f"drp3_{st}.txt")], 3)
                res[f"table3_{st}"] = as_bytes(open(f(f"drp3_{st}.txt"), "rb").read())
                print("  3 ranks vs 1 rank: table", "same" if bytes(res[f"table3_{st}"]) == table else "DIFFERENT")
    np.savez_compressed(os.path.join(OUT, f"dropan_{name}.npz"), **res)


def make_patho(exe, restate):
    import subprocess

    import dropan_strips as S
    import pathological as PG

    res, left_out = {}, []
    for name in sorted(PG.CASES):
        c = S.patho_case(O, name)
        p, fel, ad8, cols, rows, par = c["p"], c["fel"], c["ad8"], c["cols"], c["rows"], c["par"]
        ny, nx = p.shape
        dx, dy = c["dx"], c["dy"]
        gt = (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)
        one = {f"cols_{name}": cols, f"rows_{name}": rows, f"par_{name}": np.array(par, np.float64)}
        with tempfile.TemporaryDirectory() as d:
            f = lambda s: os.path.join(d, s)  # noqa: E731
            T.write_raster(f("p.tif"), p, M.P_NODATA, geotransform=gt)
            T.write_raster(f("fel.tif"), fel, float(T.FEL_NODATA), geotransform=gt)
            T.write_raster(f("ad8.tif"), ad8, -1.0, geotransform=gt)
            with open(f("outlets.txt"), "w") as fo:
                for i, (cx, r) in enumerate(zip(cols, rows)):
                    fo.write(f"{float(gt[0] + (cx + 0.5) * dx)!r} {float(gt[3] - (r + 0.5) * dy)!r} {i + 1}\n")
            try:
                for st in (0, 1):
                    args = ["-ad8", f("ad8.tif"), "-p", f("p.tif"), "-fel", f("fel.tif"), "-ssa", f("ad8.tif"), "-o", f("outlets.txt"), "-par", repr(par[0]), repr(par[1]), par[2], st]
                    stdout, _, _ = O.run_ref(exe, args + ["-drp", f(f"drp{st}.txt")], timeout=PATHO_TIMEOUT)
                    table = open(f(f"drp{st}.txt"), "rb").read()
                    one[f"table_{name}_{st}"], one[f"console_{name}_{st}"] = as_bytes(table), as_bytes(stdout.encode())
                    mine = restate.run(ad8, p, fel, ad8, cols, rows, dx, dy, par[0], par[1], par[2], st)
                    assert mine["table"] == table, f"{name} steptype {st}: the restatement's table differs from the reference's\n{mine['table'].decode()}\n{table.decode()}"
                    assert mine["console"].decode() in stdout, f"{name} steptype {st}: the restatement's console lines differ from the reference's\n{mine['console'].decode()}\n{stdout}"
                    r_ref, opt = M.parse_table(table)
                    ts = M.console_t(stdout.encode())
                    ts = ts[np.isfinite(ts)]
                    near = round(float(np.min(np.abs(np.abs(ts) - 2.0))), 4) if ts.size else None
                    print(name, p.shape, "par", par, "steptype", st, "rows", len(r_ref), "optimum", opt if mine["optimum"] is not None else None, "min ||t| - 2|", near)
            except (subprocess.TimeoutExpired, RuntimeError) as e:
                assert not np.any((p >= 1) & (p <= 8)), f"{name}: the reference failed on a raster that has flow directions: {e}"
                left_out.append(name)
                print(name, p.shape, "par", par, "the reference did not finish:", type(e).__name__, str(e)[:200].replace("\n", " "))
                continue
        res.update(one)
    print("left out:", left_out)
    np.savez_compressed(os.path.join(OUT, "dropan_patho.npz"), **res)


if __name__ == "__main__":
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_tool(tmp, "dropanalysis", ("DropAnalysis", "DropAnalysismn"))
        restate = M.compile(tmp)
        for c in M.CASES:
            if "--patho-only" not in sys.argv:
                make(exe, restate, c, ranks3=c in ("plain", "geographic"))
        make_patho(exe, restate)
