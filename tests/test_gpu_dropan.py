"""DropAnalysis on the GPU (taudem_amd/csrc/dropan.hip) against the reference's tables (tests/golden/dropan_*.npz) and against the serial restatement
(tests/dropan_model.py, held to those tables byte for byte by tests/test_dropan_restatement.py).

What is exact and what is not.  The ladder, n1, n2, every single drop, the order and elevOut of every cell, which rows are written, the total area and
the optimum are exact.  The reference adds its four float sums and its double length in the order its queue pops the cells; the GPU adds the same terms
in fp64 in a fixed order of its own.  So
  * against the goldens, DrainDen is held to 2e-6 relative (seven printed digits, the same float area, an exact-order double length), and MeanD*, StdDev*
    and T to 2 * noise + 2e-6: noise is the reference's own rounding noise per case and column, measured on the CPU by tests/golden/make_golden_dropan.py
    (its table against the table of correctly rounded sums); the factor 2 covers the second rounding when our fp64 sum becomes a float, 2e-6 is one unit
    of the %f print on each side;
  * against the restatement's drop lists, each fp64 sum is held to gamma_n * sum|x| of math.fsum (n terms, fp64 unit roundoff) and the length to
    gamma_n relative (n links and three products per row).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dropan_model as M
import dropan_rasters as DR
import taudem_amd as T
from conftest import bits_equal
from dropan_strips import check as _check, near as _near, outlets as _outlets   # shared with the strip and the pathological tests
from taudem_amd import tools

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")
RUNS = [(name, st) for name in M.CASES for st in (0, 1)]
NO_OPTIMUM = ("fourway_mask", 1)


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("dropan"))


def _golden_run(ctx, g, st, **kw):
    tmin, tmax, nt = g["par"]
    return ctx.dropanalysis(g["ad8"], g["p"], g["fel"], g["ad8"], (g["cols"], g["rows"]), thresh_min=tmin, thresh_max=tmax, nthresh=int(nt), steptype=st, dx=g["dxc"],
                            dy=g["dyc"], **kw)


# ---- goldens --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", RUNS)
def test_table_against_the_reference(ctx, name, st):
    g = M.load_golden(name)
    thresh, n1, n2, sums, length, area, table, opt = _golden_run(ctx, g, st)
    want, want_opt = M.parse_table(M.text_of(g[f"table_{st}"]))
    got, got_opt = M.parse_table(table.encode())
    print(f"{name} steptype {st}: rows {len(got)} of {len(thresh)}, optimum {opt}, total area {area}")
    assert got.shape == want.shape
    assert np.array_equal(got[:, [0, 2, 3]], want[:, [0, 2, 3]]), "ladder, n1, n2 of the written rows"
    assert got_opt == want_opt and (opt is None) == ((name, st) == NO_OPTIMUM)
    dd = np.abs(got[:, 1] - want[:, 1])
    print("  DrainDen: largest relative difference", float(np.max(dd / np.abs(want[:, 1]))))
    assert np.all(dd <= 2e-6 * np.abs(want[:, 1]))
    for c, col in enumerate(("MeanDFirstOrd", "MeanDHighOrd", "StdDevFirstOrd", "StdDevHighOrd", "T")):
        diff = float(np.max(np.abs(got[:, 4 + c] - want[:, 4 + c])))
        bound = 2.0 * float(g[f"noise_{st}"][c]) + 2e-6
        print(f"  {col}: largest difference {diff:.3g}, bound {bound:.3g}")
        assert diff <= bound, col


# ---- against the restatement ------------------------------------------------------------------------------------------------------------------
def _terrain(ctx, oracle, shape, seed, dx=30.0, dy=30.0, holes=False):
    """fel, p, ad8 of a synthetic DEM through the project's own pitremove / d8flowdir / aread8"""
    dem = oracle.synth_dem(shape, seed)
    if holes:
        rng = np.random.default_rng(seed)
        for _ in range(12):
            y, x = rng.integers(0, shape[0]), rng.integers(0, shape[1])
            dem[max(y - 3, 0):y + 4, max(x - 5, 0):x + 6] = -9999.0
    fel = ctx.pitremove(dem, -9999.0)
    p, _ = ctx.d8flowdir(fel, float(T.FEL_NODATA), dx, dy)
    ad8 = ctx.aread8(p, contcheck=False)
    return fel, p, ad8


@pytest.mark.parametrize("shape,holes", [((1, 97), False), ((97, 1), False), ((65, 67), False), ((130, 70), False), ((2048, 64), True)])
def test_random_terrain_against_the_restatement(ctx, oracle, restate, shape, holes):
    fel, p, ad8 = _terrain(ctx, oracle, shape, 11 + shape[0] + 3 * shape[1], holes=holes)
    cols, rows = _outlets(p, ad8)
    top = max(float(ad8.max()), 8.0)
    for st in (0, 1):
        ref, _ = _check(ctx, restate, ad8, p, fel, ad8, cols, rows, 30.0, 30.0, (2.0, top / 4.0, 5), st, f"{shape} steptype {st}")
    if min(shape) > 1:
        assert ref["per"][0]["n1"] > 0 and (max(shape) < 100 or ref["per"][0]["n2"] > 0)


def test_per_row_cell_sizes_against_the_restatement(ctx, oracle, restate):
    from cellsizes import rows as cell_rows

    shape = (150, 90)
    dx, dy = cell_rows("wild", shape[0], seed=5)
    fel, p, ad8 = _terrain(ctx, oracle, shape, 77, dx=dx, dy=dy)
    cols, rows = _outlets(p, ad8)
    ref, _ = _check(ctx, restate, ad8, p, fel, ad8, cols, rows, dx, dy, (2.0, 60.0, 6), 0, "150 x 90, per-row cell sizes")
    assert ref["per"][0]["n2"] > 0 and ref["per"][0]["length"] > 0


# ---- crafted rasters ----------------------------------------------------------------------------------------------------------------------------
def _crafted(ctx, restate, p, fel, ssa, what, par=(1.0, 10.0, 2), grid_th=0):
    ys, xs = np.nonzero(p == 0)                      # the network's end cell: an outlet with a direction code (0) whose downstream cell is itself
    cols, rows = xs.astype(np.int32)[:1], ys.astype(np.int32)[:1]
    return _check(ctx, restate, ssa, p, fel, ssa, cols, rows, 1.0, 1.0, par, 1, what, grid_th=grid_th)


def test_order_rule_follows_the_neighbour_scan(ctx, restate):
    """(1,1,2,2) in neighbour order gives 2, (2,2,1,1) gives 3: not Strahler's rule"""
    p, fel, ssa, ((ax, ay), (bx, by)) = DR.two_junctions()
    ref, _ = _crafted(ctx, restate, p, fel, ssa, "two junctions")
    order = ref["per"][0]["order"]
    assert order[ay, ax] == 2 and order[by, bx] == 3


def test_junctions_on_tile_corners(ctx, restate, monkeypatch):
    """inflows on both sides of the corner of the 64-cell tiles and of the 32-cell tiles, under the sweep verifier (80 x 80: the 64 x 64 geometry; the 32 x 32
    geometry runs it in test_small_tiles_in_a_process_of_their_own)"""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    p, fel, ssa, ((ax, ay), (bx, by)) = DR.tile_corners()
    ref, _ = _crafted(ctx, restate, p, fel, ssa, "tile corners")
    order = ref["per"][0]["order"]
    assert order[ay, ax] == 2 and order[by, bx] == 3


@pytest.mark.parametrize("make", [DR.off_mask_gap, DR.ssa_nodata_gap, DR.with_cycle], ids=lambda f: f.__name__)
def test_mask_edge_cases(ctx, restate, make):
    p, fel, ssa = make()
    ref, _ = _crafted(ctx, restate, p, fel, ssa, make.__name__)
    order = ref["per"][0]["order"]
    if make is DR.with_cycle:
        assert np.all(order[10, 19:22] == [1, M.ORDER_NODATA, M.ORDER_NODATA])     # the cycle's cells are never evaluated
    else:
        assert order[3, 10] == M.ORDER_NODATA and order[3, 9] > 0 and order[3, 11] == 1   # no record off the mask; the stream starts again behind the gap


def test_threshold_above_every_ssa(ctx, restate):
    p, fel, ssa = DR.off_mask_gap()
    ref, (thresh, n1, n2, sums, length, area, table, opt) = _crafted(ctx, restate, p, fel, ssa, "thresholds above every ssa", par=(20.0, 40.0, 3))
    assert not n1.any() and not n2.any() and not sums.any() and not length.any() and opt is None
    assert table == "Threshold, DrainDen, NoFirstOrd,NoHighOrd, MeanDFirstOrd, MeanDHighOrd, StdDevFirstOrd, StdDevHighOrd, T\nOptimum Threshold Value: 0.000000\n"


def test_small_tiles_in_a_process_of_their_own(ctx, restate, tmp_path):
    """The sweep reads TDX_D8_BULK_UNTIL once per process, so the 32 x 32 geometry on an 80 x 80 raster needs a process that starts with it set: the tile
    corners and a golden case, both under the sweep verifier; the results equal this process' (64 x 64 tiles) bit for bit."""
    p, fel, ssa, _ = DR.tile_corners()
    g = M.load_golden("holes")
    np.savez(tmp_path / "in.npz", p=p, fel=fel, ssa=ssa)
    code = ("import sys, json, numpy as np\n"
            f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            "import taudem_amd as T, dropan_model as M\n"
            f"a = np.load({str(tmp_path / 'in.npz')!r}); g = M.load_golden('holes')\n"
            "ys, xs = np.nonzero(a['p'] == 0)\n"
            "with T.Context(0) as c:\n"
            "    r1 = c.dropanalysis(a['ssa'], a['p'], a['fel'], a['ssa'], (xs[:1].astype(np.int32), ys[:1].astype(np.int32)), thresh_min=1.0, thresh_max=10.0, nthresh=2, steptype=1, grids=0, stats=True)\n"
            "    r2 = c.dropanalysis(g['ad8'], g['p'], g['fel'], g['ad8'], (g['cols'], g['rows']), thresh_min=3.0, thresh_max=60.0, nthresh=10, dx=g['dxc'], dy=g['dyc'], grids=4)\n"
            f"np.savez({str(tmp_path / 'out.npz')!r}, s1=r1[3], o1=r1[8], e1=r1[9], n1=r1[1], s2=r2[3], o2=r2[8], e2=r2[9], n2=r2[1])\n")
    env = dict(os.environ, TDX_D8_BULK_UNTIL="1", TDX_SWEEP_VERIFY="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.load(tmp_path / "out.npz")
    ys, xs = np.nonzero(p == 0)
    mine1 = ctx.dropanalysis(ssa, p, fel, ssa, (xs[:1].astype(np.int32), ys[:1].astype(np.int32)), thresh_min=1.0, thresh_max=10.0, nthresh=2, steptype=1, grids=0)
    mine2 = _golden_run(ctx, g, 0, grids=4)
    for tag, mine in (("1", mine1), ("2", mine2)):
        assert np.array_equal(out["n" + tag], mine[1]) and out["s" + tag].tobytes() == mine[3].tobytes()
        assert bits_equal(out["o" + tag], mine[8]) and bits_equal(out["e" + tag], mine[9])
    q = restate.threshold(p, fel, ssa, 1.0, 1.0, 1.0)
    assert bits_equal(out["o1"], q["order"]) and bits_equal(out["e1"], q["elev"])


# ---- forms and determinism ------------------------------------------------------------------------------------------------------------------------
def test_host_form_equals_device_form_and_runs_repeat(ctx):
    import torch

    g = M.load_golden("plain")
    a = _golden_run(ctx, g, 0, grids=3)
    b = _golden_run(ctx, g, 0, grids=3)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    tmin, tmax, nt = g["par"]
    d_ad8 = dev(g["ad8"])
    c = ctx.dropanalysis(d_ad8, dev(g["p"]), dev(g["fel"]), d_ad8, (g["cols"], g["rows"]), thresh_min=tmin, thresh_max=tmax, nthresh=int(nt), dx=g["dxc"], dy=g["dyc"], grids=3)
    assert c[8].is_cuda and c[9].is_cuda
    for other, what in ((b, "second run"), (c[:8] + (c[8].cpu().numpy(), c[9].cpu().numpy()), "device tensors")):
        for k in range(5):
            assert a[k].tobytes() == other[k].tobytes(), f"{what}: array {k}"
        assert a[5] == other[5] and a[6] == other[6] and a[7] == other[7], what
        assert bits_equal(a[8], other[8]) and bits_equal(a[9], other[9]), what


def test_three_strips_equal_one(ctx, oracle, restate):
    """Three strips with streams crossing both cuts: counts and grids exact, the strips' fp64 sums and lengths added in strip order within the gamma bounds of
    the one-strip result; the outlets' terms added in file order give the same total area."""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows, strip_rows

    ny, nx = 150, 110
    fel, p, ad8 = _terrain(ctx, oracle, (ny, nx), 123)
    cols, rows = _outlets(p, ad8)
    par, k = (2.0, 80.0, 5), 1
    one = ctx.dropanalysis(ad8, p, fel, ad8, (cols, rows), thresh_min=par[0], thresh_max=par[1], nthresh=par[2], dx=30.0, dy=30.0, grids=k)
    stream = ad8 >= one[0][k]
    for cut in (ny // 3, 2 * (ny // 3)):       # streams cross both cuts
        assert np.any(stream[cut - 1] & np.isin(p[cut - 1], (6, 7, 8))) or np.any(stream[cut] & np.isin(p[cut], (2, 3, 4)))
    parts = partition_rows(ny, 3)
    ts = {name: torch.from_numpy(np.ascontiguousarray(a)) for name, a in (("ad8", ad8), ("p", p), ("fel", fel))}
    with StripGroup(3, nx) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            pipe = StripPipeline(c, comm, nx, y1 - y0)
            loc = {}
            for name, t in ts.items():
                s = pipe.empty(t.dtype)
                s[1:y1 - y0 + 1].copy_(t[y0:y1])
                loc[name] = s
            ssa = loc["ad8"].clone()
            res = pipe.dropanalysis(loc["ad8"], loc["p"], loc["fel"], ssa, pipe.local_outlets(cols, rows, y0), par[0], par[1], par[2], 0, 30.0, 30.0, grids=k)
            torch.cuda.synchronize()
            return res[:6] + (res[6][1:y1 - y0 + 1].cpu().numpy(), res[7][1:y1 - y0 + 1].cpu().numpy())
        res = grp.run(rank_main)
    assert all(bits_equal(r[0], one[0]) for r in res)
    assert np.array_equal(sum(r[1] for r in res), one[1]) and np.array_equal(sum(r[2] for r in res), one[2])
    assert bits_equal(np.concatenate([r[6] for r in res]), one[8]) and bits_equal(np.concatenate([r[7] for r in res]), one[9])
    sums, length = res[0][3] + res[1][3] + res[2][3], res[0][4] + res[1][4] + res[2][4]      # strip order
    ref = restate.run(ad8, p, fel, ad8, cols, rows, 30.0, 30.0, *par, 0)
    for th, q in enumerate(ref["per"]):
        mag = M.abs_sums_from_drops(q["drops1"], q["drops2"])
        for i, nterms in enumerate((q["n1"], q["n1"], q["n2"], q["n2"])):
            assert abs(sums[th, i] - one[3][th, i]) <= 2 * M.gamma(max(nterms, 1)) * mag[i], (th, i)
        links = M.exact_length(q["order"], p, M._f64(30.0, ny), M._f64(30.0, ny))[1]
        assert abs(length[th] - one[4][th]) <= 2 * M.gamma(links + 3 * ny) * one[4][th], th
    term = res[0][5] + res[1][5] + res[2][5]                                                # one strip owns an outlet, the others say 0
    ta = np.float32(0.0)
    for t in term:                                                                          # file order
        ta = np.float32(ta + t)
    assert np.float32(float(ta) * 30.0 * 30.0) == one[5] and one[5] > 0
    assert ref["per"][0]["n2"] > 0


# ---- command line and module ---------------------------------------------------------------------------------------------------------------------------
def _write_case(tmp_path, g, name="plain"):
    f = lambda s: str(tmp_path / s)  # noqa: E731
    dx, dy, geo = float(g["dx"]), float(g["dy"]), bool(g["geographic"])
    ny = g["p"].shape[0]
    gt = (-111.9, dx, 0.0, 41.9, 0.0, -dy) if geo else (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)
    T.write_raster(f("p.tif"), g["p"], M.P_NODATA, geotransform=gt, geographic=geo)
    T.write_raster(f("fel.tif"), g["fel"], float(T.FEL_NODATA), geotransform=gt, geographic=geo)
    T.write_raster(f("ad8.tif"), g["ad8"], -1.0, geotransform=gt, geographic=geo)
    with open(f("outlets.txt"), "w") as fo:
        for i, (c, r) in enumerate(zip(g["cols"], g["rows"])):
            fo.write(f"{float(gt[0] + (c + 0.5) * dx)!r} {float(gt[3] - (r + 0.5) * dy)!r} {i + 1}\n")
    return f, gt


@pytest.mark.parametrize("name", ["plain", "geographic"])
def test_cli_and_tools_write_the_context_table(ctx, tmp_path, name):
    g = M.load_golden(name)
    f, _ = _write_case(tmp_path, g)
    tmin, tmax, nt = g["par"]
    table = _golden_run(ctx, g, 0)[6].encode()
    opt = M.parse_table(table)[1]
    base = ["-ad8", f("ad8.tif"), "-p", f("p.tif"), "-fel", f("fel.tif"), "-ssa", f("ad8.tif"), "-o", f("outlets.txt"), "-par", repr(float(tmin)), repr(float(tmax)), str(int(nt)), "0"]
    for gpus in (1, 2):
        r = subprocess.run([os.path.join(BIN, "dropanalysis"), "--gpus", str(gpus), *base, "-drp", f(f"drp{gpus}.txt")], capture_output=True, text=True, timeout=180)
        assert r.returncode == 0 and "DropAnalysis version" in r.stdout and f"Processes: {gpus}" in r.stdout, r.stdout + r.stderr
        assert "Threshold DrainDen NoFirstOrd" in r.stdout and f"{opt:f}  Value for optimum that drop analysis selected" in r.stdout
        assert "This run may take on the order of 1 minutes to complete." in r.stderr
        got = open(f(f"drp{gpus}.txt"), "rb").read()
        assert got == table if gpus == 1 else _near(got, table, g["noise_0"]), got.decode() + table.decode()
    rc, topt = tools.dropan(f("ad8.tif"), f("p.tif"), f("fel.tif"), f("ad8.tif"), f("drpm.txt"), f("outlets.txt"), threshmin=tmin, threshmax=tmax, nthresh=int(nt), steptype=0)
    assert rc == 0 and f"{topt:f}" == f"{opt:f}" and open(f("drpm.txt"), "rb").read() == table


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, tmp_path):
    g = M.load_golden("plain")
    f, gt = _write_case(tmp_path, g)
    args = (f("ad8.tif"), f("p.tif"), f("fel.tif"), f("ad8.tif"))
    # fewer than two thresholds
    with pytest.raises(ValueError):
        ctx.dropanalysis(g["ad8"], g["p"], g["fel"], g["ad8"], (g["cols"], g["rows"]), nthresh=1)
    assert tools.dropan(*args, f("t1.txt"), f("outlets.txt"), nthresh=1)[0] == 7 and not os.path.exists(f("t1.txt"))
    # an outlet on a cell without a direction
    ys, xs = np.nonzero(g["p"] == M.P_NODATA)
    bad = (np.append(g["cols"], xs[0]).astype(np.int32), np.append(g["rows"], ys[0]).astype(np.int32))
    with pytest.raises(T.TdxError) as e:
        ctx.dropanalysis(g["ad8"], g["p"], g["fel"], g["ad8"], bad)
    assert e.value.code == -1 and "lies on a cell without a flow direction" in str(e.value)
    with open(f("bad.txt"), "w") as fo:
        fo.write(open(f("outlets.txt")).read() + f"{float(gt[0] + (xs[0] + 0.5) * float(g['dx']))!r} {float(gt[3] - (ys[0] + 0.5) * float(g['dy']))!r} 99\n")
    assert tools.dropan(*args, f("t2.txt"), f("bad.txt"))[0] == -1 and not os.path.exists(f("t2.txt"))
    # no outlets
    with pytest.raises(ValueError):
        ctx.dropanalysis(g["ad8"], g["p"], g["fel"], g["ad8"], None)
    assert tools.dropan(*args, f("t3.txt"), "")[0] == 5 and not os.path.exists(f("t3.txt"))
    r = subprocess.run([os.path.join(BIN, "dropanalysis"), "-ad8", args[0], "-p", args[1], "-fel", args[2], "-ssa", args[3], "-drp", f("t4.txt")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0 and "-o <outletsshapefile> is required" in r.stdout and "Use with specific file names" in r.stdout and not os.path.exists(f("t4.txt"))
    r = subprocess.run([os.path.join(BIN, "dropanalysis"), "-ad8", args[0], "-p", args[1], "-fel", args[2], "-ssa", args[3], "-o", f("outlets.txt"), "-drp", f("t4.txt"), "-par",
                        "2", "40"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("\nUse with specific file names") and not os.path.exists(f("t4.txt"))   # a -par that is cut short
    # rasters of different sizes
    T.write_raster(f("small.tif"), g["p"][:-3], M.P_NODATA, geotransform=gt)
    assert tools.dropan(args[0], f("small.tif"), args[2], args[3], f("t5.txt"), f("outlets.txt"))[0] == 4 and not os.path.exists(f("t5.txt"))
    with pytest.raises(ValueError):
        ctx.dropanalysis(g["ad8"], g["p"][:-3].copy(), g["fel"], g["ad8"], (g["cols"], g["rows"]))
