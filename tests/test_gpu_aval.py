"""RetLimFlow and DinfAvalanche on the GPU (taudem_amd/csrc/dinfaval.hip): Context.retlimflow / Context.dinfavalanche and the two command-line
tools against the reference's rasters (tests/golden/aval_*.npz), and against the C restatement of tests/aval_model.py (held to those goldens
by tests/test_aval_restatement.py) at sizes and cell geometries the goldens do not cover: ragged shapes around the 64-cell tile, per-row
`wild` cell sizes, 2048 x 2048, both tile geometries under the sweep verifier, three strips.

qrl is compared bit for bit.  rz: the reference calls the host's float atan (glibc documents 1 ulp), the device evaluates atan in double and
rounds once (0.5 ulp), and * 180 / PI with the final rounding adds at most 1 ulp: outside the cells aval_model marks as tainted - a decision
that close that such an error could flip it, or a contributor that is tainted - rz must agree within 3 float ulps (derived, not measured),
and dfs and the set of cells with data bit for bit.  The tainted cells must stay below 1 % of the runout in every input used here, so that
a broken kernel cannot hide behind the mask (aval_model.compare_aval asserts both)."""
import os
import subprocess

import numpy as np
import pytest

import aval_model as M
import taudem_amd as T
from cellsizes import rows
from conftest import bits_equal, describe_diff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")


def same(a, b, name):
    assert bits_equal(a, b), describe_diff(a, b, name)


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("aval"))


def _inputs(ctx, oracle, shape, seed, dx=30.0, dy=30.0, holes=False):
    """(ang, fel, wg, rc): angles of a pit-filled synthetic DEM with a few cells without a direction (-1) and without an angle, a few nodata
    elevations under valid angles, runoff / retention grids with nodata cells and blocks where the retention wins."""
    rng = np.random.default_rng(seed)
    dem = oracle.synth_dem(shape, seed)
    ny, nx = shape
    if holes and ny > 8 and nx > 8:
        for _ in range(max(1, ny * nx // 40000)):
            y, x = rng.integers(0, ny - 4), rng.integers(0, nx - 4)
            dem[y:y + rng.integers(2, 12), x:x + rng.integers(2, 12)] = -9999.0
    fel = ctx.pitremove(dem, -9999.0)
    ang, _ = ctx.dinfflowdir(fel, -3.0e38, dx, dy)
    ang, fel = ang.copy(), fel.copy()
    valid = ang > -1e30
    ang[valid & (rng.random(shape) < 0.002)] = -1.0
    ang[rng.random(shape) < 0.001] = M.ANG_NODATA
    fel[rng.random(shape) < 0.002] = M.FEL_NODATA
    wg = (rng.random(shape, dtype=np.float32) * 4.0).astype(np.float32)
    rc = rng.random(shape, dtype=np.float32)
    for _ in range(max(1, ny * nx // 20000)):
        y, x = rng.integers(0, max(ny - 8, 1)), rng.integers(0, max(nx - 8, 1))
        rc[y:y + 10, x:x + 10] += 30.0
    wg[rng.random(shape) < 0.0005] = M.WG_NODATA
    rc[rng.random(shape) < 0.0005] = M.RC_NODATA
    return ang, fel, wg, rc


def _sources(shape, seed, density):
    rng = np.random.default_rng(seed)
    ass = np.zeros(shape, np.int16)
    ass[rng.random(shape) < density] = 1
    ass[rng.random(shape) < density / 4] = M.ASS_NODATA
    if ass.size > 200:
        y, x = rng.integers(0, shape[0] - 2), rng.integers(0, max(shape[1] - 3, 1))
        ass[y:y + 2, x:x + 3] = 3
    return ass


# Uniform cells of 30 x 40: the diagonal is 50, every path length is an integer and exact in float, so two paths of equal length from one source
# give the SAME record and no near-tie (on 10 x 12.5 cells the two orders of one straight and one diagonal step round differently, and
# 10 - 30 % of a runout is tainted: measured with the restatement alone).  Per-row cell sizes have no such choice: there the seed search
# of _check_aval picks sources whose runouts have few such confluences.
PYTH = (30.0, 40.0)
RUNS = ((False, M.DEFAULT), (True, M.DEFAULT), (False, M.OTHER), (True, M.OTHER))


def _check_aval(ctx, restate, ang, fel, dx, dy, what, seed=1, density=0.004, runs=RUNS, geo=None, geographic=False):
    """Source cells for which the tainted share stays small (the restatement alone decides, before the GPU is asked: near-ties between two
    paths from one source are a property of the terrain), then every run under the rule of the module docstring."""
    ny = ang.shape[0]
    for s in range(seed, seed + 12):
        ass = _sources(ang.shape, s, density)
        refs = [restate.dinfavalanche(ang, fel, ass, thresh=ta[0], alpha=ta[1], direct=d, dxc=dx, dyc=dy, geo=geo, geographic=geographic) for d, ta in runs]
        if all(t.sum() <= 0.8 * M.MAX_TAINT_SHARE * max(int((rz > -1e30).sum()), 1) for rz, _, t in refs):
            break
    bad = []
    for (d, ta), (rrz, rdfs, taint) in zip(runs, refs):
        rz, dfs = ctx.dinfavalanche(ang, fel, ass, thresh=ta[0], alpha=ta[1], direct=d, dx=dx, dy=dy, geo=geo, geographic=geographic)
        bad += M.compare_aval(rz, dfs, rrz, rdfs, taint, f"{what}, {'direct' if d else 'path'} thresh {ta[0]} alpha {ta[1]}")
    assert not bad, "\n".join(bad)
    assert ny == 1 or any((rz > -1e30).sum() > 0 for rz, _, _ in refs) or ang.size < 4000, f"{what}: no runout at all"
    return ass


def _check_retlim(ctx, restate, ang, wg, rc, dx, dy, what):
    same(ctx.retlimflow(ang, wg, rc, dx=dx, dy=dy), restate.retlimflow(ang, wg, rc, dxc=dx, dyc=dy), f"qrl, {what}")


@pytest.mark.parametrize("name", M.golden_names())
def test_context_matches_reference_goldens(ctx, restate, name):
    g = M.load_golden(name)
    same(ctx.retlimflow(g["ang"], g["wg"], g["rc"], dx=g["dxc"], dy=g["dyc"]), g["qrl"], f"{name}: qrl")
    geo, geographic = M.golden_geo(g)
    bad = []
    for sfx, direct, ta in M.variants():
        _, _, taint = M.run_aval(restate, g, direct, ta)
        rz, dfs = ctx.dinfavalanche(g["ang"], g["fel"], g["ass"], thresh=ta[0], alpha=ta[1], direct=direct, dx=g["dxc"], dy=g["dyc"], geo=geo, geographic=geographic)
        bad += M.compare_aval(rz, dfs, g["rz" + sfx], g["dfs" + sfx], taint, f"{name}{sfx}")
    assert not bad, "\n".join(bad)


def test_device_tensors(ctx, restate):
    import torch

    g = M.load_golden("holes")
    dev = f"cuda:{ctx.device}"
    t = {k: torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in ("ang", "fel", "ass", "wg", "rc")}
    same(ctx.retlimflow(t["ang"], t["wg"], t["rc"], dx=g["dxc"], dy=g["dyc"]).cpu().numpy(), g["qrl"], "qrl on device tensors")
    geo, geographic = M.golden_geo(g)
    bad = []
    for sfx, direct, ta in M.variants()[:2]:
        _, _, taint = M.run_aval(restate, g, direct, ta)
        rz, dfs = ctx.dinfavalanche(t["ang"], t["fel"], t["ass"], thresh=ta[0], alpha=ta[1], direct=direct, dx=g["dxc"], dy=g["dyc"], geo=geo, geographic=geographic)
        bad += M.compare_aval(rz.cpu().numpy(), dfs.cpu().numpy(), g["rz" + sfx], g["dfs" + sfx], taint, f"device tensors{sfx}")
    assert not bad, "\n".join(bad)
    with pytest.raises(ValueError):
        ctx.retlimflow(t["ang"], g["wg"], t["rc"])


def test_direct_refuses_a_raster_wider_than_65536(ctx):
    nx = 65537
    ang = np.zeros((1, nx), np.float32)
    fel = np.ones((1, nx), np.float32)
    ass = np.zeros((1, nx), np.int16)
    with pytest.raises(T.TdxError, match="65536"):
        ctx.dinfavalanche(ang, fel, ass, direct=True)
    rz, _ = ctx.dinfavalanche(ang, fel, ass)   # the path mode has no such limit
    assert rz.shape == (1, nx)


def test_a_nodata_angle_that_sends(ctx, restate):
    """ang nodata = -1 on cells 2.5 times as tall as wide: atan2(dy, dx) > 1, so prop() of the nodata value is positive towards the east and
    the reference adds such a neighbour's never-written qrl (-FLT_MAX) although nothing waits for it."""
    g = M.load_golden("rect_dxdy")
    ang = g["ang"].copy()
    ang[ang < -1e30] = -1.0
    ref = restate.retlimflow(ang, g["wg"], g["rc"], dxc=g["dxc"], dyc=g["dyc"], ang_nodata=-1.0)
    assert not bits_equal(ref, restate.retlimflow(g["ang"], g["wg"], g["rc"], dxc=g["dxc"], dyc=g["dyc"]))
    same(ctx.retlimflow(ang, g["wg"], g["rc"], dx=g["dxc"], dy=g["dyc"], nodata=-1.0), ref, "qrl with ang nodata -1 on 10 x 25 cells")


@pytest.mark.parametrize("shape", [(1, 1), (1, 97), (97, 1), (63, 63), (64, 64), (65, 65), (63, 65), (65, 64), (64, 129), (130, 63)])
def test_restatement_ragged_shapes(ctx, oracle, restate, shape):
    ang, fel, wg, rc = _inputs(ctx, oracle, shape, 5 + shape[0] * 7 + shape[1], dx=PYTH[0], dy=PYTH[1])
    _check_retlim(ctx, restate, ang, wg, rc, *PYTH, f"{shape[0]} x {shape[1]}")
    _check_aval(ctx, restate, ang, fel, *PYTH, f"{shape[0]} x {shape[1]}", seed=shape[0] + shape[1], density=0.02)


@pytest.mark.parametrize("shape", [(257, 301), (65, 64), (700, 96)])
def test_restatement_wild_cell_sizes(ctx, oracle, restate, shape):
    dx, dy = rows("wild", shape[0], seed=shape[1])
    ang, fel, wg, rc = _inputs(ctx, oracle, shape, 23 + shape[1], dx=dx, dy=dy)
    _check_retlim(ctx, restate, ang, wg, rc, dx, dy, f"{shape[0]} x {shape[1]} wild rows")
    _check_aval(ctx, restate, ang, fel, dx, dy, f"{shape[0]} x {shape[1]} wild rows", seed=shape[1], density=0.01)


@pytest.mark.slow
def test_2048_under_the_sweep_verifier(ctx, oracle, restate, monkeypatch):
    """2048 x 2048: the bulk rounds on 32 x 32 tiles hand over to 64 x 64 tiles, and TDX_SWEEP_VERIFY=1 re-evaluates every swept cell from its
    contributors' final records with the policy's own expression."""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    ang, fel, wg, rc = _inputs(ctx, oracle, (2048, 2048), 31, dx=PYTH[0], dy=PYTH[1], holes=True)
    _check_retlim(ctx, restate, ang, wg, rc, *PYTH, "2048 x 2048")
    _check_aval(ctx, restate, ang, fel, *PYTH, "2048 x 2048", seed=77, density=0.0005, runs=RUNS[:2])


def _run(tool, *args):
    r = subprocess.run([os.path.join(BIN, tool), *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("name", M.golden_names())
@pytest.mark.parametrize("ngpus", [1, 3])
def test_cli_matches_reference_goldens(tmp_path, restate, name, ngpus):
    g = M.load_golden(name)
    ny = g["ang"].shape[0]
    (xleft, ytop, dx, dy), geographic = M.golden_geo(g)
    gt = (xleft, dx, 0.0, ytop, 0.0, -dy)
    f = lambda s: str(tmp_path / s)  # noqa: E731
    for key, nd in (("ang", M.ANG_NODATA), ("fel", M.FEL_NODATA), ("wg", M.WG_NODATA), ("rc", M.RC_NODATA), ("ass", M.ASS_NODATA)):
        T.write_raster(f(f"b{key}.tif"), g[key], nd, geotransform=gt, geographic=geographic)   # the simple form's names: nameadd("b.tif", suffix)
    N = ["--gpus", str(ngpus)]
    out = _run("retlimflow", *N, "-ang", f("bang.tif"), "-wg", f("bwg.tif"), "-rc", f("brc.tif"), "-qrl", f("q.tif"))
    assert "Retention limited flow accumulation version" in out and f"Processors: {min(ngpus, ny)}" in out
    same(T.read_raster(f("q.tif"), np.float32)[0], g["qrl"], f"{name}: retlimflow --gpus {ngpus}")
    _run("retlimflow", *N, f("b.tif"))
    same(T.read_raster(f("bqrl.tif"), np.float32)[0], g["qrl"], f"{name}: retlimflow simple form --gpus {ngpus}")
    bad = []
    for sfx, direct, (thresh, alpha) in M.variants():
        _, _, taint = M.run_aval(restate, g, direct, (thresh, alpha))
        extra = ([] if (thresh, alpha) == M.DEFAULT else ["-thresh", str(thresh), "-alpha", str(alpha)]) + (["-direct"] if direct else [])
        out = _run("dinfavalanche", *N, "-ang", f("bang.tif"), "-fel", f("bfel.tif"), "-ass", f("bass.tif"), "-rz", f("rz.tif"), "-dfs", f("dfs.tif"), *extra)
        assert "DinfAvalanche version" in out and f"Processors: {min(ngpus, ny)}" in out
        bad += M.compare_aval(T.read_raster(f("rz.tif"), np.float32)[0], T.read_raster(f("dfs.tif"), np.float32)[0], g["rz" + sfx], g["dfs" + sfx], taint,
                              f"{name}: dinfavalanche {' '.join(extra)} --gpus {ngpus}")
    _run("dinfavalanche", *N, f("b.tif"))   # simple form: defaults, path mode
    _, _, taint = M.run_aval(restate, g, False, M.DEFAULT)
    bad += M.compare_aval(T.read_raster(f("brz.tif"), np.float32)[0], T.read_raster(f("bdfs.tif"), np.float32)[0], g["rz_path"], g["dfs_path"], taint,
                          f"{name}: dinfavalanche simple form --gpus {ngpus}")
    assert not bad, "\n".join(bad)


@pytest.mark.slow
def test_three_strips_equal_one_gpu(ctx, oracle, restate):
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows, strip_rows

    ny, nx = 1500, 1300
    dx, dy = rows("wild", ny, seed=3)
    ang, fel, wg, rc = _inputs(ctx, oracle, (ny, nx), 41, dx=dx, dy=dy, holes=True)
    geo = (500.0, 9000.0, 7.0, 5.0)
    runs = RUNS[:2]
    ass = _check_aval(ctx, restate, ang, fel, dx, dy, "1500 x 1300 wild rows, one GPU", seed=9, density=0.001, runs=runs, geo=geo)
    one_q = ctx.retlimflow(ang, wg, rc, dx=dx, dy=dy)
    one = [ctx.dinfavalanche(ang, fel, ass, thresh=ta[0], alpha=ta[1], direct=d, dx=dx, dy=dy, geo=geo) for d, ta in runs]
    parts = partition_rows(ny, 3)
    ts = {k: torch.from_numpy(v) for k, v in (("ang", ang), ("fel", fel), ("wg", wg), ("rc", rc), ("ass", ass))}
    with StripGroup(3, nx) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            pipe = StripPipeline(c, comm, nx, y1 - y0)
            loc = {}
            for k, t in ts.items():
                s = pipe.empty(t.dtype)
                s[1:y1 - y0 + 1].copy_(t[y0:y1])
                loc[k] = s
            sdx, sdy = strip_rows(dx, y0, y1), strip_rows(dy, y0, y1)
            q, _ = pipe.retlimflow(loc["ang"], loc["wg"], loc["rc"], dx=sdx, dy=sdy)
            torch.cuda.synchronize()
            res = [q[1:y1 - y0 + 1].cpu().numpy()]
            for d, ta in runs:
                rz, dfs, _ = pipe.dinfavalanche(loc["ang"], loc["fel"], loc["ass"], row0=y0, ny_total=ny, thresh=ta[0], alpha=ta[1], direct=d, dx=sdx, dy=sdy, geo=geo)
                torch.cuda.synchronize()
                res += [rz[1:y1 - y0 + 1].cpu().numpy(), dfs[1:y1 - y0 + 1].cpu().numpy()]
            return res
        res = grp.run(rank_main)
    same(np.concatenate([r[0] for r in res]), one_q, "qrl in three strips")
    for i, (d, ta) in enumerate(runs):   # the same kernel on the same records: strips against one GPU bit for bit
        same(np.concatenate([r[1 + 2 * i] for r in res]), one[i][0], f"rz {'direct' if d else 'path'} in three strips")
        same(np.concatenate([r[2 + 2 * i] for r in res]), one[i][1], f"dfs {'direct' if d else 'path'} in three strips")
