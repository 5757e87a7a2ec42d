"""DropAnalysis in row strips (StripPipeline.dropanalysis, taudem_amd/csrc/dropan.hip with the forward D8 sweep of d8_sweep.hpp) under arbitrary cuts, against
the serial restatement OF THE WHOLE RASTER with the global per-row cell sizes (tests/dropan_model.py, held to the reference byte for byte by
tests/test_dropan_restatement.py).  The inputs are the CPU oracle's, so that a wrong direction raster cannot hide a wrong DropAnalysis; every run is under
the sweep verifier.  tests/dropan_strips.py has the strip runner, the combination of the strips' numbers and the assertions (assert_strips: what is exact
and what is bounded is said there); tests/test_dropan_strips_model.py shows on the CPU that those assertions notice a planted error, and that the inputs
chosen here meet the conditions asked of them (rows of the table, margin of every |t| to 2, junctions on cut rows) by the restatement alone.

The random cuts as the restatement gives them on the CPU (log ladder (2, max ssa / 4, 6) / arithmetic ladder (2, 27, 6)):

    seed  raster     strips (owned rows)        sizes  ssa   rows   min ||t| - 2|     junctions on cut rows
    0     205 x 300  15 25 47 118               const  ad8   5 / 6  0.0892 / 2.7855   270
    1     205 x 306  28 44 90 43                wild   pd    4 / 6  0.8490 / 1.0068    37
    2     206 x 301  31 1 94 80                 band   ad8   5 / 6  0.6385 / 1.9338   183
    3     207 x 301  38 142 17 10               const  pd    4 / 6  0.4013 / 0.1154    36
    4     208 x 302  154 54                     wild   ad8   4 / 6  1.6952 / 3.1380    88
    5     205 x 308  1 123 57 23 1              band   pd    4 / 6  0.2274 / 0.0487    33
    6     205 x 308  12 41 114 38               const  ad8   5 / 6  1.5212 / 4.7488   294
    7     204 x 306  34 2 59 51 8 50            wild   pd    5 / 6  0.0423 / 0.7261    48

n2 of the first written row is 356 to 3036.  On an MI355X a seed (both step types) takes 0.15 to 0.18 s, the first one 1.8 s; a crafted case 0.01 s; the
command-line test 0.4 s."""
import os
import subprocess

import numpy as np
import pytest

import dropan_model as M
import dropan_rasters as DR
import dropan_strips as S
import peuker_model as PM
import taudem_amd as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")
CLI_SEED = 6      # constant cell sizes (seed % 3 == 0), ssa = ad8


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("dropan"))


@pytest.fixture(scope="module")
def peuker(tmp_path_factory):
    return PM.compile(tmp_path_factory.mktemp("peuker"))


def _run(restate, ad8, p, fel, ssa, cols, rows, parts, dx, dy, par, st, grid_th, what, ssa_nodata=-1.0):
    """the strips on the device, their combination, and assert_strips against the restatement of the whole raster"""
    ref = restate.run(ad8, p, fel, ssa, cols, rows, dx, dy, par[0], par[1], par[2], st, ssa_nodata=ssa_nodata)
    results, comb = S.in_strips((ad8, p, fel, ssa), parts, dx, dy, (cols, rows), par, st, grid_th, ssa_nodata=ssa_nodata)
    S.assert_strips(results, comb, ref, p, fel, parts, dx, dy, grid_th, what)
    return ref, results, comb


# ---- a. random cuts -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", S.SEEDS)
def test_random_cuts_against_the_restatement(oracle, restate, peuker, monkeypatch, seed):
    c = S.random_case(oracle, peuker, seed)
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    monkeypatch.setenv("TDX_SWEEP_EAGER_ROUNDS", str(c["eager"]))
    sizes = [y1 - y0 for y0, y1 in c["parts"]]
    assert seed != S.ONE_ROW_SEED or 1 in sizes
    assert seed != S.EDGE_SEED or (c["parts"][0] == (0, 1) and c["parts"][-1] == (c["ny"] - 1, c["ny"]))
    for st in (0, 1):
        par = S.ladder_of(c["ssa"], st)
        what = f"seed {seed}, steptype {st}, {c['ny']} x {c['nx']} in {c['parts']}"
        ref, _, _ = _run(restate, c["ad8"], c["p"], c["fel"], c["ssa"], c["cols"], c["rows"], c["parts"], c["dx"], c["dy"], par, st, c["grid_th"], what)
        nrows, n2_first, margin, on_cut = S.input_conditions(ref, c["p"], c["parts"])
        print(f"{what}: {nrows} rows, n2 of the first {n2_first}, min ||t| - 2| {margin:.4f}, {on_cut} junctions on cut rows")
        assert nrows >= 4 and n2_first > 0 and margin > 0.01 and on_cut >= 1, what


# ---- b. junctions on the cut, crafted ---------------------------------------------------------------------------------------------------------------
def _crafted(restate, p, fel, ssa, parts, what):
    ys, xs = np.nonzero(p == 0)                      # the network's end cell, as in tests/test_gpu_dropan.py
    cols, rows = xs.astype(np.int32)[:1], ys.astype(np.int32)[:1]
    return _run(restate, ssa, p, fel, ssa, cols, rows, parts, 1.0, 1.0, (1.0, 10.0, 2), 1, 0, what)


TWO_JUNCTION_CUTS = [[(0, 10), (10, 21)],                 # the junctions on the first owned row, their N arms in the halo
                     [(0, 11), (11, 21)],                 # ... on the last owned row, their S arms in the halo
                     [(0, 10), (10, 11), (11, 21)],       # a one-row strip that owns only the junctions' row
                     [(0, 9), (9, 12), (12, 21)]]


@pytest.mark.parametrize("parts", TWO_JUNCTION_CUTS, ids=lambda v: "-".join(str(a) for a, _ in v[1:]))
def test_two_junctions_on_the_cut(restate, monkeypatch, parts):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    p, fel, ssa, ((ax, ay), (bx, by)) = DR.two_junctions()
    ref, results, _ = _crafted(restate, p, fel, ssa, parts, f"two junctions in {parts}")
    order = ref["per"][0]["order"]
    assert order[ay, ax] == 2 and order[by, bx] == 3
    # row 10 holds both junctions and the heads of the order-2 arms that run along it (W of the first, E of the second: two sources meet, two first-order
    # drops each).  (1,1,2,2) -> 2: two first-order drops; (2,2,1,1) -> 3: two first-order and two higher-order drops.  Row 10: 8 and 2.  The strip that
    # owns row 10 reports exactly the drops of its rows, at both thresholds.
    owner = next(r for r, (y0, y1) in enumerate(parts) if y0 <= ay < y1)
    (jy, _, jo, _), _ = S.junction_drops(order, ref["per"][0]["elev"], p, fel)
    assert (int(np.sum((jy == ay) & (jo == 1))), int(np.sum((jy == ay) & (jo != 1)))) == (8, 2)
    own_rows = range(*parts[owner])
    want = (int(np.sum(np.isin(jy, own_rows) & (jo == 1))), int(np.sum(np.isin(jy, own_rows) & (jo != 1))))
    for th in range(2):
        assert (int(results[owner][1][th]), int(results[owner][2][th])) == want, (owner, th)
        if parts[owner] == (ay, ay + 1):
            assert want == (8, 2)            # the one-row strip: exactly the drops of row 10 (the N and S arms' heads belong to its neighbours)


def test_tile_corner_junctions_on_the_cuts(restate, monkeypatch):
    """the junctions at (64, 64) and (32, 32), each on the only row of a one-row strip: all their inflows from the N side lie in a halo row"""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    p, fel, ssa, ((ax, ay), (bx, by)) = DR.tile_corners()
    parts = [(0, 32), (32, 33), (33, 64), (64, 65), (65, 80)]
    ref, results, _ = _crafted(restate, p, fel, ssa, parts, "tile corners cut at 32, 33, 64, 65")
    order = ref["per"][0]["order"]
    assert order[ay, ax] == 2 and order[by, bx] == 3
    assert S.junctions_on_cut_rows(order, p, parts) >= 2


@pytest.mark.parametrize("make", [DR.off_mask_gap, DR.ssa_nodata_gap, DR.with_cycle], ids=lambda f: f.__name__)
def test_mask_edge_cases_on_the_cuts(restate, monkeypatch, make):
    """cut at rows 3, 4, 6 and 10: the stream rows 3 and 6 and the cycle's row 10 are each the first or the last row of a strip"""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    p, fel, ssa = make()
    parts = [(0, 3), (3, 4), (4, 6), (6, 10), (10, 12)]
    ref, _, _ = _crafted(restate, p, fel, ssa, parts, f"{make.__name__} cut at 3, 4, 6, 10")
    order = ref["per"][0]["order"]
    if make is DR.with_cycle:
        assert np.all(order[10, 19:22] == [1, M.ORDER_NODATA, M.ORDER_NODATA])
    else:
        assert order[3, 10] == M.ORDER_NODATA and order[3, 9] > 0 and order[3, 11] == 1
    assert S.junctions_on_cut_rows(order, p, parts) >= 1


# ---- c. the command line in three strips ----------------------------------------------------------------------------------------------------------------
def test_cli_in_three_strips_equals_one_device(ctx, oracle, restate, peuker, tmp_path):
    """`dropanalysis --gpus 3` on the rasters of one random case at constant cell sizes: its table against the one-device table, DrainDen within 2e-6
    relative and every other column within the 2e-6 of the %f print (near() with no noise allowance: both tables come from fp64 sums).  Measured on
    an MI355X: the two tables are the same in every printed digit (largest difference 0 in all six columns, five rows)."""
    c = S.random_case(oracle, peuker, CLI_SEED)
    dx, dy = c["dx"], c["dy"]
    assert isinstance(dx, float) and c["ssa"] is c["ad8"]
    ny = c["ny"]
    f = lambda s: str(tmp_path / s)  # noqa: E731
    gt = (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)
    T.write_raster(f("p.tif"), c["p"], M.P_NODATA, geotransform=gt)
    T.write_raster(f("fel.tif"), c["fel"], float(T.FEL_NODATA), geotransform=gt)
    T.write_raster(f("ad8.tif"), c["ad8"], -1.0, geotransform=gt)
    with open(f("outlets.txt"), "w") as fo:
        for i, (x, y) in enumerate(zip(c["cols"], c["rows"])):
            fo.write(f"{float(gt[0] + (x + 0.5) * dx)!r} {float(gt[3] - (y + 0.5) * dy)!r} {i + 1}\n")
    par = S.ladder_of(c["ssa"], 0)
    one = ctx.dropanalysis(c["ad8"], c["p"], c["fel"], c["ad8"], (c["cols"], c["rows"]), thresh_min=par[0], thresh_max=par[1], nthresh=par[2], steptype=0, dx=dx, dy=dy)
    table = one[6].encode()
    ref = restate.run(c["ad8"], c["p"], c["fel"], c["ad8"], c["cols"], c["rows"], dx, dy, *par, 0)
    assert S.same_tables(table, ref["table"]) and len(M.parse_table(table)[0]) >= 4
    r = subprocess.run([os.path.join(BIN, "dropanalysis"), "--gpus", "3", "-ad8", f("ad8.tif"), "-p", f("p.tif"), "-fel", f("fel.tif"), "-ssa", f("ad8.tif"), "-o", f("outlets.txt"),
                        "-par", repr(par[0]), repr(par[1]), str(par[2]), "0", "-drp", f("drp3.txt")], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "Processes: 3" in r.stdout, r.stdout + r.stderr
    got = open(f("drp3.txt"), "rb").read()
    a, b = M.parse_table(got), M.parse_table(table)
    if a[0].shape == b[0].shape and len(a[0]):
        print("largest differences per column (DrainDen relative):", float(np.max(np.abs(a[0][:, 1] - b[0][:, 1]) / np.abs(b[0][:, 1]))), np.max(np.abs(a[0][:, 4:] - b[0][:, 4:]), axis=0))
    assert S.near(got, table, np.zeros(5)), got.decode() + table.decode()
