"""CatchHydroGeo and InunDepth on the GPU (taudem_amd/csrc/handtools.hip): Context.catchhydrogeo / .inundepth, the strip entry points, the two tool
functions and the two command-line tools against the reference's outputs (tests/golden/hand_*.npz) and the C restatement of tests/hand_model.py
(held to those goldens byte for byte by tests/test_hand_restatement.py).

Counts are compared exactly.  The fp64 sums are compared with the EXACT sum (math.fsum over the terms as the reference evaluates them): a sum of n
terms in any order is within gamma_n * sum|term|, gamma_n = (n-1)u / (1 - (n-1)u), u = 2^-53, of it; the same is asserted of the restatement, so
the reference's own order is shown to sit inside the bound.  The depth raster is compared bit for bit."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hand_model as M
import taudem_amd as T
from conftest import bits_equal, describe_diff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")
CASES = ("fourway_mask", "geographic", "holes", "plain", "rect_dxdy")
STAGES = np.array([0.5, 0.0, 1.0, 2.0, 1.0, 3.0, 5.0, 4.0, 8.0, 12.0, 20.0, 40.0])
KEYS = ("surface", "bed", "volume")


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("hand"))


def _within(got, exact, sumabs, n, what, extra=0.0):
    """|got - exact| <= gamma_n * sum|term| (+ extra), entry by entry; prints the worst ratio before it asserts."""
    g = np.vectorize(M.gamma)(n)
    bound = g * sumabs + extra
    err = np.abs(np.asarray(got, np.float64) - exact)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)))) if err.size else 0.0
    print(f"{what}: worst |err| / bound = {worst:.3g}")
    assert np.all(err <= bound), f"{what}: {int(np.sum(err > bound))} entries outside the bound, worst ratio {worst}"


def check_sums(res, ref, exact, what):
    """res / ref: (count, surface, bed, volume, catcharea) of the GPU and of the restatement; exact: hand_model.exact_sums()."""
    ex, count, ca = exact
    assert np.array_equal(res[0], count.astype(np.int32)), f"{what}: count"
    assert np.array_equal(ref[0], count.astype(np.int32)), f"{what}: restatement count"
    for who, r in (("gpu", res), ("restatement", ref)):
        for i, key in enumerate(KEYS):
            _within(r[1 + i], ex[key][0], ex[key][1], count, f"{what}: {who} {key}")
        _within(r[4], ca[0], ca[1], ca[2], f"{what}: {who} catcharea")


def seeded(shape, seed, nseeds=6, ids=None, zero=True):
    """hand (some cells exactly 0, +-5e-7, nodata), catch (Voronoi, 1 % nodata), slp (a few nodata) for a shape."""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    hand = rng.gamma(1.5, 3.0, shape).astype(np.float32)
    slp = rng.uniform(0.0, 0.8, shape).astype(np.float32)
    cat = M.voronoi(ny, nx, nseeds, seed + 1, ids)
    if zero and ny * nx >= 64:
        pick = rng.choice(ny * nx, 12, replace=False)
        hand.flat[pick[:4]] = 0.0
        hand.flat[pick[4:6]] = 5e-7
        hand.flat[pick[6:8]] = -5e-7
        hand.flat[pick[8:10]] = M.HAND_NODATA
        slp.flat[pick[10:]] = M.SLP_NODATA
        cat.flat[np.flatnonzero(rng.random(ny * nx) < 0.01)] = M.CATCH_NODATA
    return hand, cat, slp


def run_both(ctx, restate, hand, cat, slp, ids, stages, dx, dy, what):
    ny = hand.shape[0]
    res = ctx.catchhydrogeo(hand, cat, slp, ids, stages, dx=dx, dy=dy)
    ref = restate.chg_sums(hand, cat, slp, dx, dy, ids, stages)
    check_sums(res, ref, M.exact_sums(hand, cat, slp, np.broadcast_to(dx, (ny,)), np.broadcast_to(dy, (ny,)), ids, stages), what)
    return res


@pytest.mark.parametrize("name", CASES)
def test_catchhydrogeo_on_the_goldens(ctx, restate, tmp_path, name):
    g = M.load_golden(name)
    (tmp_path / "list.csv").write_bytes(M.text_of(g["list_csv"]))
    (tmp_path / "stages.txt").write_bytes(M.text_of(g["stages_txt"]))
    ids = restate.read_list(str(tmp_path / "list.csv"))[0]
    stages = restate.read_stages(str(tmp_path / "stages.txt"))
    run_both(ctx, restate, g["hand"], g["catch"], g["slp"], ids, stages, g["dxc"], g["dyc"], name)


SHAPES = [(1, 1), (1, 200), (200, 1), (63, 65), (65, 130), (257, 193)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_catchhydrogeo_small_shapes(ctx, restate, shape):
    ids = np.array([4, -9, 70000, 4, 12, 3, 8], np.int32)          # 4 twice: the second row wins; 8 is not in the raster
    hand, cat, slp = seeded(shape, 100 + shape[0], 6, [4, -9, 70000, 12, 3, 555])
    run_both(ctx, restate, hand, cat, slp, ids, STAGES, 30.0, 25.0, f"voronoi {shape}")
    ny, nx = shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    for edge in (64, 50):                                          # catchment borders on and off the tile edges
        blocks = ((yy // edge) * 8 + xx // edge + 1).astype(np.int32)
        run_both(ctx, restate, hand, blocks, slp, np.arange(1, 41, dtype=np.int32), STAGES, 30.0, 25.0, f"blocks of {edge} {shape}")


def test_one_catchment_covers_512x512(ctx, restate):
    hand, _, slp = seeded((512, 512), 7, 1)
    cat = np.full((512, 512), 17, np.int32)
    res = run_both(ctx, restate, hand, cat, slp, np.array([17], np.int32), STAGES, 10.0, 10.0, "one catchment")   # ncatch = 1: 64 records in one list
    again = ctx.catchhydrogeo(hand, cat, slp, np.array([17], np.int32), STAGES, dx=10.0, dy=10.0)
    for a, b in zip(res, again):                                   # two runs: the same bits
        assert a.tobytes() == b.tobytes()
    run_both(ctx, restate, hand, cat, slp, np.array([17], np.int32), np.array([2.5]), 10.0, 10.0, "ncatch 1, nheight 1")


def test_83_stages_on_512x512(ctx, restate):
    hand, cat, slp = seeded((512, 512), 8, 40)
    stages = np.round(np.linspace(0.0, 25.0, 83), 3)
    res = run_both(ctx, restate, hand, cat, slp, np.arange(1, 41, dtype=np.int32), stages, 30.0, 30.0, "83 stages")
    again = ctx.catchhydrogeo(hand, cat, slp, np.arange(1, 41, dtype=np.int32), stages, dx=30.0, dy=30.0)
    for a, b in zip(res, again):
        assert a.tobytes() == b.tobytes()


def test_checkerboard_of_unique_ids(ctx, restate):
    """Every cell of 128 x 128 has its own listed id: 4096 distinct ids per tile."""
    rng = np.random.default_rng(9)
    hand, _, slp = seeded((128, 128), 9, 1, zero=False)
    ids = rng.permutation(128 * 128).astype(np.int32) * 3 - 20000
    cat = ids.reshape(128, 128).copy()
    res = run_both(ctx, restate, hand, cat, slp, ids, np.array([1.0, 4.0, 0.0]), 30.0, 30.0, "checkerboard")
    assert np.all(res[4] == 900.0)


def test_long_list_few_used(ctx, restate):
    rng = np.random.default_rng(10)
    ids = (rng.permutation(200000)[:50000] - 100000).astype(np.int32)
    hand, cat, slp = seeded((96, 80), 10, 7, ids[[5, 49999, 12345, 0, 777, 31000, 2]])
    res = run_both(ctx, restate, hand, cat, slp, ids, STAGES, 30.0, 30.0, "50 000 ids")
    assert np.count_nonzero(res[4]) == 7


def test_nothing_listed_and_nothing_there(ctx, restate):
    hand, cat, slp = seeded((70, 90), 11, 5)
    res = run_both(ctx, restate, hand, cat, slp, np.array([1000, 2000], np.int32), STAGES, 30.0, 30.0, "unlisted")
    assert not any(np.any(r) for r in res)
    cat[:] = M.CATCH_NODATA
    res = run_both(ctx, restate, hand, cat, slp, np.arange(1, 6, dtype=np.int32), STAGES, 30.0, 30.0, "all nodata")
    assert not any(np.any(r) for r in res)


def test_stage_chunks_give_the_same_bits(ctx, restate, monkeypatch):
    """A slab budget of 1 KiB forces one stage per launch (TDX_CHG_SLAB_MB): every entry keeps its bits, whatever the chunking."""
    hand, cat, slp = seeded((200, 260), 13, 9)
    ids = np.arange(1, 10, dtype=np.int32)
    whole = run_both(ctx, restate, hand, cat, slp, ids, STAGES, 30.0, 30.0, "one chunk")
    monkeypatch.setenv("TDX_CHG_SLAB_MB", "0.001")
    *chunked, st = ctx.catchhydrogeo(hand, cat, slp, ids, STAGES, dx=30.0, dy=30.0, stats=True)
    assert st["rounds"] == STAGES.size
    for a, b in zip(whole, chunked):
        assert a.tobytes() == b.tobytes()


def test_per_row_cell_sizes(ctx, restate):
    ny, nx = 130, 70
    lat = np.deg2rad(41.0 - 0.01 * np.arange(ny))
    dxc, dyc = 111320.0 * 0.0003 * np.cos(lat), np.full(ny, 110574.0 * 0.0003) + 1e-3 * np.arange(ny)
    hand, cat, slp = seeded((ny, nx), 12, 5)
    run_both(ctx, restate, hand, cat, slp, np.arange(1, 6, dtype=np.int32), STAGES, dxc, dyc, "geographic rows")


def _strips(ctx, hand, cat, slp, dxc, dyc, ids, stages, cuts):
    """The strip entry point on device arrays of nyl + 2 rows, one strip after the other; the partial tables added in strip order."""
    import ctypes as C

    import torch

    ny, nx = hand.shape
    ids, stages = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(stages, np.float64)
    nc, nh = ids.size, stages.size
    tot = [np.zeros((nh, nc), np.int32)] + [np.zeros((nh, nc)) for _ in range(3)] + [np.zeros(nc)]
    v = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for y0, y1 in zip([0] + cuts, cuts + [ny]):
        def strip(a, fill):
            s = np.full((y1 - y0 + 2, nx), fill, a.dtype)
            s[1:-1] = a[y0:y1]
            return torch.from_numpy(s).to(f"cuda:{ctx.device}")
        th, tc, ts = strip(hand, 0), strip(cat, 1), strip(slp, 0)      # halo rows hold listed ids: they must not be counted
        rows = np.clip(np.arange(y0 - 1, y1 + 1), 0, ny - 1)
        sdx, sdy = np.ascontiguousarray(dxc[rows]), np.ascontiguousarray(dyc[rows])
        part = [np.zeros((nh, nc), np.int32)] + [np.zeros((nh, nc)) for _ in range(3)] + [np.zeros(nc)]
        torch.cuda.synchronize(ctx.device)
        T._lib.check(ctx._lib.tdx_catchhydrogeo_strip(ctx._h, None, th.data_ptr(), tc.data_ptr(), ts.data_ptr(), nx, y1 - y0, float(M.HAND_NODATA), int(M.CATCH_NODATA),
                                                      float(M.SLP_NODATA), v(sdx), v(sdy), v(ids), nc, v(stages), nh, *(v(p) for p in part), None), ctx._h)
        for t, p in zip(tot, part):
            t += p
    return tot


@pytest.mark.parametrize("seed", [1, 2])
def test_strips_with_random_cuts(ctx, restate, seed):
    rng = np.random.default_rng(500 + seed)
    ny, nx = 200, 150
    hand, cat, slp = seeded((ny, nx), 20 + seed, 6)
    ids = np.arange(1, 7, dtype=np.int32)
    dxc, dyc = np.full(ny, 30.0) + 0.01 * np.arange(ny), np.full(ny, 28.0)
    cuts = sorted(int(c) for c in rng.choice(np.arange(1, ny), 3, replace=False))
    got = _strips(ctx, hand, cat, slp, dxc, dyc, ids, STAGES, cuts)
    ref = restate.chg_sums(hand, cat, slp, dxc, dyc, ids, STAGES)
    check_sums(got, ref, M.exact_sums(hand, cat, slp, dxc, dyc, ids, STAGES), f"strips cut at {cuts}")


def test_strips_of_one_row(ctx, restate):
    """Every strip one row tall (what --gpus 8 makes of a short raster): both halo rows of a strip are its neighbours' only owned rows."""
    ny, nx = 12, 150
    hand, cat, slp = seeded((ny, nx), 23, 6)
    ids = np.arange(1, 7, dtype=np.int32)
    dxc, dyc = np.full(ny, 30.0) + 0.01 * np.arange(ny), np.full(ny, 28.0)
    got = _strips(ctx, hand, cat, slp, dxc, dyc, ids, STAGES, list(range(1, ny)))
    ref = restate.chg_sums(hand, cat, slp, dxc, dyc, ids, STAGES)
    check_sums(got, ref, M.exact_sums(hand, cat, slp, dxc, dyc, ids, STAGES), "12 strips of one row")


def _write_rasters(d, g):
    gt, geo = tuple(g["gt"]), bool(g["geographic"])
    f = lambda s: os.path.join(str(d), s)  # noqa: E731
    T.write_raster(f("hand.tif"), g["hand"], M.HAND_NODATA, geotransform=gt, geographic=geo)
    T.write_raster(f("slp.tif"), g["slp"], M.SLP_NODATA, geotransform=gt, geographic=geo)
    T.write_raster(f("catch.tif"), g["catch"], M.CATCH_NODATA, geotransform=gt, geographic=geo)
    T.write_raster(f("mask.tif"), g["mask"], M.MASK_NODATA, geotransform=gt, geographic=geo)
    for key, name in (("list_csv", "list.csv"), ("stages_txt", "stages.txt"), ("fc_csv", "fc.csv"), ("table_txt", "table.txt")):
        open(f(name), "wb").write(M.text_of(g[key]))
    return f


def compare_tables(got, want, exact, lst):
    """Field by field against the restatement's (= the reference's) text: id, stage, count, slope, length, n as text; the sums within the bound of
    the exact sum + 5e-7 of print rounding; the derived columns within (5/3) gamma_V + (2/3) gamma_B + 8u relative + 5e-7 of the value derived from
    the exact sums (flow ~ V^(5/3) B^(-2/3)); the zero pattern of the guards equal to the reference's.  lst: (ids, slope, length, n)."""
    ex, count, ca = exact
    ids, slope, length, mann = lst
    ncatch = ids.size
    gl, wl = got.strip().split("\n"), want.strip().split("\n")
    assert gl[0] == wl[0] and len(gl) == len(wl)
    nh = (len(gl) - 1) // ncatch
    for r, (a, b) in enumerate(zip(gl[1:], wl[1:])):
        a, b = a.split(","), b.split(",")
        c, k = r // nh, r % nh
        for col in (0, 1, 2, 6, 7, 12):
            assert a[col] == b[col], (r, col, a, b)
        gam = M.gamma(int(count[k, c]))
        for col, key in ((3, "surface"), (4, "bed"), (5, "volume")):
            assert abs(float(a[col]) - ex[key][0][k, c]) <= gam * ex[key][1][k, c] + 5e-7, (r, col, a, b)
        assert abs(float(a[8]) - ca[0][c]) <= M.gamma(int(ca[2][c])) * ca[1][c] + 5e-7, (r, a, b)
        vol, bed = ex["volume"][0][k, c], ex["bed"][0][k, c]
        xs = wp = hr = q = 0.0
        if vol > 0:
            if length[c] > 0:
                xs, wp = vol / length[c], bed / length[c]
            if wp > 0:
                hr = xs / wp
                q = (xs * hr ** (2.0 / 3.0) * math.sqrt(slope[c])) / mann[c]
        rel = (5.0 / 3.0) * gam + (2.0 / 3.0) * gam + 8 * M.U        # gamma_V and gamma_B share n
        for col, d in ((9, xs), (10, wp), (11, hr), (13, q)):
            assert (float(a[col]) == 0.0) == (float(b[col]) == 0.0), (r, col, a, b)
            assert abs(float(a[col]) - d) <= rel * abs(d) + 5e-7, (r, col, a, b, d)


@pytest.mark.parametrize("name", ["plain", "geographic", "rect_dxdy"])
def test_tool_functions_on_files(ctx, restate, tmp_path, name):
    from taudem_amd import tools

    g = M.load_golden(name)
    f = _write_rasters(tmp_path, g)
    lst = restate.read_list(f("list.csv"))
    ids = lst[0]
    stages = restate.read_stages(f("stages.txt"))
    assert tools.catchhydrogeo(f("hand.tif"), f("catch.tif"), f("list.csv"), f("slp.tif"), f("stages.txt"), f("out.txt")) == 0
    exact = M.exact_sums(g["hand"], g["catch"], g["slp"], g["dxc"], g["dyc"], ids, stages)
    compare_tables(open(f("out.txt")).read(), M.text_of(g["table_txt"]).decode(), exact, lst)
    # InunDepth from the REFERENCE's table, so that the depths are the reference's
    for masked in (False, True):
        assert tools.inundepth(f("hand.tif"), f("catch.tif"), f("mask.tif") if masked else None, f("fc.csv"), f("table.txt"), f("map.tif"), f("depth.csv")) == 0
        m, _ = T.read_raster(f("map.tif"), np.float32)
        want = g["map_mask" if masked else "map"]
        assert bits_equal(m, want), describe_diff(m, want, f"{name}: map")
        compare_depths(open(f("depth.csv")).read(), M.text_of(g["depth_csv"]).decode(), g, restate, f)


def wet_cells(g, ids, depth):
    """Per forecast row: (n, exact area) of the cells the inundated area counts, at the winning row of each id."""
    hand, cat = g["hand"], g["catch"]
    ny, nx = hand.shape
    area = np.repeat((g["dxc"] * g["dyc"])[:, None], nx, 1)
    win = {int(v): i for i, v in enumerate(ids)}
    out = {}
    nd = np.abs((hand - np.float32(M.HAND_NODATA)).astype(np.float32)) < np.float32(1e-5)
    for v, i in win.items():
        d = np.float32(depth[i])
        m = (cat == v) & ~nd & (cat != M.CATCH_NODATA) & bool(d > 0) & ((d - hand).astype(np.float32) > 0)
        out[i] = (int(m.sum()), math.fsum(area[m]))
    return out


def compare_depths(got, want, g, restate, f):
    """id, flow, depth and CatchArea as text; the -9999 pattern equal; InunArea within n 2^-24 of the exact area, relative, plus the print rounding,
    for the GPU's row and for the reference's.  n, not n - 1: the terms are doubles, so the first add into the float accumulator rounds as well
    (one catchment cell of a geographic raster already shows it); the GPU's fp64 sum rounded once has the single 2^-24."""
    ids, flow, depth, carea = restate.inun_depths(f("fc.csv"), f("table.txt"))
    wet = wet_cells(g, ids, depth)
    win = {int(v): i for i, v in enumerate(ids)}
    gl, wl = got.strip().split("\n"), want.strip().split("\n")
    assert gl[0] == wl[0] and len(gl) == len(wl)
    for r, (a, b) in enumerate(zip(gl[1:], wl[1:])):
        a, b = a.split(","), b.split(",")
        assert a[:3] == b[:3] and a[4] == b[4], (a, b)                       # id, flow, depth, CatchArea: as text
        n, exact = wet[win[int(a[0])]]
        rel = max(n - 1, 0) * 2.0 ** -24
        for who, row in (("gpu", a), ("reference", b)):
            assert (row[3] == "-9999.000000") == (exact <= 0) and (row[5] == "-9999.000000") == (b[5] == "-9999.000000"), (who, row)
            if exact > 0:
                # (n-1) 2^-24: the reference's running float sum; + 2^-24 for the final rounding to float, + the print rounding
                assert abs(float(row[3]) - exact) <= (rel + 2.0 ** -24) * exact + 5e-7, (who, row, exact)
                if row[5] != "-9999.000000":
                    ratio = exact / float(row[4])
                    assert abs(float(row[5]) - ratio) <= (rel + 2.0 ** -24 + 2.0 ** -23) * ratio + 5e-7, (who, row, ratio)


@pytest.mark.parametrize("name", CASES)
def test_inundepth_arrays_on_the_goldens(ctx, restate, tmp_path, name):
    g = M.load_golden(name)
    f = _write_rasters(tmp_path, g)
    ids, flow, depth, carea = restate.inun_depths(f("fc.csv"), f("table.txt"))
    m, area = ctx.inundepth(g["hand"], g["catch"], ids, depth, dx=g["dxc"], dy=g["dyc"])
    assert bits_equal(m, g["map"]), describe_diff(m, g["map"], name)
    mm, _ = ctx.inundepth(g["hand"], g["catch"], ids, depth, mask=g["mask"], area=False)
    assert bits_equal(mm, g["map_mask"]) and np.all(mm == M.MAP_NODATA)
    wet = wet_cells(g, ids, depth)
    ref = restate.inun_area(g["hand"], g["catch"], g["dxc"], g["dyc"], ids, depth)
    for i in range(ids.size):
        n, exact = wet.get(i, (0, 0.0))
        for who, a in (("gpu", area), ("restatement", ref)):
            assert abs(float(a[i]) - exact) <= (max(n - 1, 0) + 1) * 2.0 ** -24 * exact, (who, i, float(a[i]), exact)


@pytest.mark.parametrize("shape", [(1, 1), (1, 200), (200, 1), (65, 130), (257, 193)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_inundepth_threshold_to_the_ulp(ctx, restate, shape):
    """Cells planted at hfc - hand = 0.001 -+ 1 ulp of hand, depths <= 0 and ids without a depth; bit for bit against the restatement."""
    ny, nx = shape
    hand, cat, _ = seeded(shape, 300 + ny, 5, [3, -8, 41, 500, 77])
    ids = np.array([3, -8, 41, 3, 77, 9], np.int32)
    depth = np.array([9.0, 2.25, -9999.0, 4.5, 0.0, 1.0], np.float32)
    base = np.float32(4.5 - 0.001)
    plant = [base, np.nextafter(base, np.float32(-1e9)), np.nextafter(base, np.float32(1e9)), np.float32(4.5), np.float32(0.0)]
    cells = np.flatnonzero(cat == 3)[:len(plant)]
    hand.flat[cells] = plant[:cells.size]
    m, area = ctx.inundepth(hand, cat, ids, depth, dx=30.0, dy=20.0)
    want = restate.inun_map(hand, cat, ids, depth)
    assert bits_equal(m, want), describe_diff(m, want, str(shape))
    ref = restate.inun_area(hand, cat, 30.0, 20.0, ids, depth)
    assert np.all(np.abs(area.astype(np.float64) - ref) <= (ny * nx) * 2.0 ** -24 * np.maximum(area, ref)), (area, ref)
    assert np.array_equal(area == 0, ref == 0)
    mm, _ = ctx.inundepth(hand, cat, ids, depth, mask=np.zeros(shape, np.int16), area=False)
    assert np.all(mm == M.MAP_NODATA)


def test_error_paths(ctx, tmp_path, capfd):
    from taudem_amd import tools

    g = M.load_golden("plain")
    f = _write_rasters(tmp_path, g)
    T.write_raster(f("short.tif"), g["catch"][:-3].copy(), M.CATCH_NODATA)
    assert tools.catchhydrogeo(f("hand.tif"), f("short.tif"), f("list.csv"), f("slp.tif"), f("stages.txt"), f("o.txt")) == 1     # size mismatch
    assert tools.inundepth(f("hand.tif"), f("short.tif"), None, f("fc.csv"), f("table.txt"), f("m.tif")) == 1
    capfd.readouterr()
    assert tools.catchhydrogeo(f("hand.tif"), f("catch.tif"), f("nolist.csv"), f("slp.tif"), f("stages.txt"), f("o.txt")) == 1
    assert "ERROR: Cannot open catch list file!" in capfd.readouterr().err
    open(f("two.csv"), "w").write("id,slope\n7,0.01\n")
    assert tools.catchhydrogeo(f("hand.tif"), f("catch.tif"), f("two.csv"), f("slp.tif"), f("stages.txt"), f("o.txt")) == 1
    assert "ERROR: Catchment list file must have at least 3 columns (id, slope, length)." in capfd.readouterr().err
    assert not os.path.exists(f("o.txt"))


@pytest.mark.parametrize("gpus", [1, 2])
def test_command_line_tools(restate, tmp_path, gpus):
    g = M.load_golden("holes")
    f = _write_rasters(tmp_path, g)
    r = subprocess.run([os.path.join(BIN, "catchhydrogeo"), "--gpus", str(gpus), "-hand", f("hand.tif"), "-catch", f("catch.tif"), "-catchlist", f("list.csv"), "-slp",
                        f("slp.tif"), "-h", f("stages.txt"), "-table", f("out.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "CatchHydroGeo version 5.4.0" and re.fullmatch(r"Compute time: \d+\.\d{6}", lines[-1]), r.stdout
    lst = restate.read_list(f("list.csv"))
    exact = M.exact_sums(g["hand"], g["catch"], g["slp"], g["dxc"], g["dyc"], lst[0], restate.read_stages(f("stages.txt")))
    compare_tables(open(f("out.txt")).read(), M.text_of(g["table_txt"]).decode(), exact, lst)
    r = subprocess.run([os.path.join(BIN, "inundepth"), "--gpus", str(gpus), "-hand", f("hand.tif"), "-catch", f("catch.tif"), "-fc", f("fc.csv"), "-hp", f("table.txt"),
                        "-inun", f("map.tif"), "-depth", f("depth.csv")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "InunDepth version 5.4.0" and re.fullmatch(r"Inundation depth Compute time: \d+\.\d{6}", lines[-1]), r.stdout
    m, _ = T.read_raster(f("map.tif"), np.float32)
    assert bits_equal(m, g["map"]), describe_diff(m, g["map"], "map")
    compare_depths(open(f("depth.csv")).read(), M.text_of(g["depth_csv"]).decode(), g, restate, f)
