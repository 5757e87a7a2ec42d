"""D8HDistToStrm and GageWatershed on the GPU (taudem_amd/csrc/d8rev.hip): Context.d8hdisttostrm / Context.gagewatershed and the two
command-line tools against the reference's outputs (tests/golden/d8rev_*.npz: two -src / -thresh runs, the gauge raster and the -id file),
and against the C restatement of tests/d8rev_model.py (held to those goldens by tests/test_d8rev_restatement.py) at sizes and cell
geometries the goldens do not cover: ragged shapes around the tile edges, per-row cell sizes, nodata holes and long flow paths, both tile
geometries under the sweep verifier, three strips with gauges on the strip-boundary rows, device tensors."""
import os
import subprocess

import numpy as np
import pytest

import d8rev_model as M
import taudem_amd as T
from cellsizes import rows
from conftest import bits_equal, describe_diff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")
SRC_ND = -2147483647


def same(a, b, name):
    assert bits_equal(a, b), describe_diff(a, b, name)


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("d8rev"))


def _inputs(ctx, oracle, shape, seed, dx=30.0, dy=30.0, holes=False, gauge_rows=()):
    """(p, src, ad8, (cols, rows, ids)): D8 directions of a pit-filled synthetic DEM with a few p == 0 cells, src = 1 on the top 6 % of AreaD8
    with nodata holes (int32, nodata SRC_ND), AreaD8 as int32, and gauges on large-area cells (some on `gauge_rows`) with shuffled ids,
    plus one off the raster and a second one on a taken cell."""
    rng = np.random.default_rng(seed)
    ny, nx = shape
    dem = oracle.synth_dem(shape, seed)
    if holes and ny > 8 and nx > 8:
        for _ in range(max(1, ny * nx // 40000)):
            y, x = rng.integers(0, ny - 4), rng.integers(0, nx - 4)
            dem[y:y + rng.integers(2, 12), x:x + rng.integers(2, 12)] = -9999.0
    fel = ctx.pitremove(dem, -9999.0)
    p, _ = ctx.d8flowdir(fel, -3.0e38, dx, dy)
    p = p.copy()
    ad8 = ctx.aread8(p)
    ad8i = np.where(ad8 < -0.5, SRC_ND, np.rint(ad8)).astype(np.int32)
    p[(rng.random(shape) < 0.002) & (p > 0)] = 0
    valid = ad8i != SRC_ND
    src = np.zeros(shape, np.int32)
    if valid.any():
        src[valid & (ad8i >= np.quantile(ad8i[valid], 0.94))] = 1
    src[rng.random(shape) < 0.003] = SRC_ND
    big = np.flatnonzero(ad8i.ravel() >= np.quantile(ad8i, 0.9)) if valid.any() else np.arange(ny * nx)
    picks = list(rng.choice(big, min(12, big.size), replace=False))
    for r in gauge_rows:
        r = min(max(int(r), 0), ny - 1)
        picks.append(r * nx + int(np.argmax(ad8i[r])))
    cols = [int(c % nx) for c in picks] + [nx + 3, int(picks[0] % nx)]
    rws = [int(c // nx) for c in picks] + [ny // 2, int(picks[0] // nx)]
    ids = rng.permutation(10 * len(cols))[:len(cols)].astype(np.int32) + 1
    return p, src, ad8i, (np.array(cols, np.int32), np.array(rws, np.int32), ids)


def _check(ctx, restate, p, src, ad8i, gauges, dx, dy, what):
    for s, th, tag in ((src, 1, "src"), (ad8i, 200, "ad8 -thresh 200")):
        out = ctx.d8hdisttostrm(p, s, th, dx=dx, dy=dy, src_nodata=SRC_ND)
        same(out, restate.dist(p, s, th, dx, dy, src_nodata=SRC_ND), f"dist {tag}, {what}")
    gw, table = ctx.gagewatershed(p, gauges)
    gw_ref, text = restate.gage(p, *gauges)
    assert np.array_equal(gw, gw_ref), f"{what}: {int(np.sum(gw != gw_ref))} gauge labels differ"
    assert M.table_text(table) == text, what


@pytest.mark.parametrize("name", M.golden_names())
def test_context_matches_reference_goldens(ctx, name):
    g = M.load_golden(name)
    out = ctx.d8hdisttostrm(g["p"], g["src"], dx=g["dxc"], dy=g["dyc"], src_nodata=int(g["src_nodata"]))
    same(out, g["dist_src"], f"{name}: -src src")
    out = ctx.d8hdisttostrm(g["p"], g["ad8"], M.THRESH_AD8, dx=g["dxc"], dy=g["dyc"], src_nodata=int(g["ad8_nodata"]))
    same(out, g["dist_ad8"], f"{name}: -src ad8 -thresh {M.THRESH_AD8}")
    gw, table = ctx.gagewatershed(g["p"], (g["cols"], g["rows"], g["ids"]))
    assert np.array_equal(gw, g["gw"]), f"{name}: {int(np.sum(gw != g['gw']))} gauge labels differ"
    assert M.table_text(table) == str(g["id_text"]), name


def test_device_tensors(ctx):
    import torch

    g = M.load_golden("holes")
    dev = f"cuda:{ctx.device}"
    p, src = (torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in ("p", "src"))
    out = ctx.d8hdisttostrm(p, src, dx=g["dxc"], dy=g["dyc"], src_nodata=int(g["src_nodata"]))
    assert out.is_cuda
    same(out.cpu().numpy(), g["dist_src"], "device tensors: dist")
    gw, table = ctx.gagewatershed(p, (g["cols"], g["rows"], g["ids"]))
    assert gw.is_cuda and np.array_equal(gw.cpu().numpy(), g["gw"])
    assert M.table_text(table) == str(g["id_text"])


@pytest.mark.parametrize("shape", [(1, 1), (1, 97), (97, 1), (31, 33), (32, 32), (33, 31), (63, 63), (64, 64), (65, 65), (63, 65), (64, 129), (130, 63)])
def test_restatement_ragged_shapes(ctx, oracle, restate, shape):
    p, src, ad8i, gauges = _inputs(ctx, oracle, shape, 5 + shape[0] * 7 + shape[1])
    _check(ctx, restate, p, src, ad8i, gauges, 10.0, 12.5, f"{shape[0]} x {shape[1]}")


@pytest.mark.parametrize("kind,shape", [("wild", (257, 301)), ("wild", (65, 64)), ("band", (700, 96)), ("fine", (300, 200))])
def test_restatement_per_row_cell_sizes(ctx, oracle, restate, kind, shape):
    dx, dy = rows(kind, shape[0], seed=shape[1])
    p, src, ad8i, gauges = _inputs(ctx, oracle, shape, 23 + shape[1], dx=dx, dy=dy)
    _check(ctx, restate, p, src, ad8i, gauges, dx, dy, f"{shape[0]} x {shape[1]} {kind} rows")


def test_restatement_2048_with_holes(ctx, oracle, restate):
    p, src, ad8i, gauges = _inputs(ctx, oracle, (2048, 2176), 17, holes=True)
    _check(ctx, restate, p, src, ad8i, gauges, 30.0, 30.0, "2048 x 2176 with holes")


def test_large_under_the_sweep_verifier(ctx, oracle, restate, monkeypatch):
    """3100 x 2900: the bulk rounds on 32 x 32 tiles hand over to 64 x 64 tiles, and TDX_SWEEP_VERIFY=1 re-evaluates every swept cell
    from its receiver's final record with the policy's own expression."""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    p, src, ad8i, gauges = _inputs(ctx, oracle, (3100, 2900), 31, holes=True)
    _check(ctx, restate, p, src, ad8i, gauges, 30.0, 30.0, "3100 x 2900 under the verifier")


def test_three_strips_equal_restatement(ctx, oracle, restate):
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows, strip_rows

    ny, nx = 1500, 1300
    parts = partition_rows(ny, 3)
    cut = [y for y0, y1 in parts for y in (y0 - 1, y0, y1 - 1, y1) if 0 <= y < ny]
    dx, dy = rows("wild", ny, seed=3)
    p, src, ad8i, gauges = _inputs(ctx, oracle, (ny, nx), 41, dx=dx, dy=dy, holes=True, gauge_rows=cut)
    ref_dist = restate.dist(p, src, 1, dx, dy, src_nodata=SRC_ND)
    ref_gw, ref_text = restate.gage(p, *gauges)
    ts = {"p": torch.from_numpy(p), "src": torch.from_numpy(src)}
    with StripGroup(3, nx) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            pipe = StripPipeline(c, comm, nx, y1 - y0)
            loc = {}
            for k, t in ts.items():
                s = pipe.empty(t.dtype)
                s[1:y1 - y0 + 1].copy_(t[y0:y1])
                loc[k] = s
            dist, _ = pipe.d8hdisttostrm(loc["p"], loc["src"], 1, dx=strip_rows(dx, y0, y1), dy=strip_rows(dy, y0, y1), src_nodata=SRC_ND)
            lc, lr = pipe.local_outlets(gauges[0], gauges[1], y0)
            gw, table, _ = pipe.gagewatershed(loc["p"], (lc, lr, gauges[2]))
            torch.cuda.synchronize()
            return dist[1:y1 - y0 + 1].cpu().numpy(), gw[1:y1 - y0 + 1].cpu().numpy(), table
        res = grp.run(rank_main)
    same(np.concatenate([r[0] for r in res]), ref_dist, "dist in three strips")
    gw = np.concatenate([r[1] for r in res])
    assert np.array_equal(gw, ref_gw), f"{int(np.sum(gw != ref_gw))} gauge labels differ in three strips"
    for r in res:
        assert M.table_text(r[2]) == ref_text


def _run(tool, *args, ok=True):
    r = subprocess.run([os.path.join(BIN, tool), *args], capture_output=True, text=True, timeout=120)
    if ok:
        assert r.returncode == 0, r.stdout + r.stderr
    return r


@pytest.mark.parametrize("name", M.golden_names())
@pytest.mark.parametrize("ngpus", [1, 3])
def test_cli_matches_reference_goldens(tmp_path, name, ngpus):
    g = M.load_golden(name)
    gt, geo = tuple(float(v) for v in g["gt"]), bool(g["geographic"])
    dx, dy = gt[1], -gt[5]
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("bp.tif"), g["p"], M.P_NODATA, geotransform=gt, geographic=geo)   # the simple form's names: nameadd("b.tif", suffix)
    T.write_raster(f("bsrc.tif"), g["src"].astype(np.int16), int(g["src_nodata"]), geotransform=gt, geographic=geo)
    T.write_raster(f("ad8.tif"), g["ad8"], int(g["ad8_nodata"]), geotransform=gt, geographic=geo)
    with open(f("gauges.txt"), "w") as fo:   # tests/golden/make_golden_d8rev.py
        for c, r, i in zip(g["cols"], g["rows"], g["ids"]):
            fo.write(f"{float(gt[0] + (c + 0.5) * dx)!r} {float(gt[3] - (r + 0.5) * dy)!r} {i}\n")
    N = ["--gpus", str(ngpus)]
    out = _run("d8hdisttostrm", *N, "-p", f("bp.tif"), "-src", f("bsrc.tif"), "-dist", f("d1.tif")).stdout
    assert "D8HDistToStrm version" in out and f"Processors: {ngpus}" in out
    same(T.read_raster(f("d1.tif"), np.float32)[0], g["dist_src"], f"{name}: d8hdisttostrm --gpus {ngpus}")
    _run("d8hdisttostrm", *N, "-p", f("bp.tif"), "-src", f("ad8.tif"), "-thresh", str(M.THRESH_AD8), "-dist", f("d2.tif"))
    same(T.read_raster(f("d2.tif"), np.float32)[0], g["dist_ad8"], f"{name}: d8hdisttostrm -thresh --gpus {ngpus}")
    _run("d8hdisttostrm", *N, f("b.tif"))   # simple form: nameadd suffixes p, src, dist; -thresh 1
    same(T.read_raster(f("bdist.tif"), np.float32)[0], g["dist_src"], f"{name}: simple form --gpus {ngpus}")
    out = _run("gagewatershed", *N, "-p", f("bp.tif"), "-o", f("gauges.txt"), "-gw", f("gw.tif"), "-id", f("id.txt"), "-lyrno", "0").stdout
    assert "Gage Watershed version" in out and f"Size: {ngpus}" in out
    gw, _ = T.read_raster(f("gw.tif"), np.int32)
    assert np.array_equal(gw, g["gw"]), f"{name}: gagewatershed --gpus {ngpus}"
    with open(f("id.txt")) as fi:
        assert fi.read() == str(g["id_text"])


def test_cli_refuses_upid(tmp_path):
    g = M.load_golden("plain")
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("p.tif"), g["p"], M.P_NODATA)
    with open(f("gauges.txt"), "w") as fo:
        fo.write("10.5 20.5 1\n")
    r = _run("gagewatershed", "-p", f("p.tif"), "-o", f("gauges.txt"), "-gw", f("gw.tif"), "-upid", f("up.txt"), ok=False)
    assert r.returncode != 0 and "-upid is not supported" in r.stderr
    assert not os.path.exists(f("gw.tif")) and not os.path.exists(f("up.txt"))
    from taudem_amd import tools

    assert tools.gagewatershed(f("p.tif"), f("gw2.tif"), f("gauges.txt"), writeupid=1, upidfile=f("up.txt")) != 0
