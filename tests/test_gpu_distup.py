"""DinfDistUp on the GPU (taudem_amd/csrc/dinfdistup.hip): Context.dinfdistup and the dinfdistup command-line tool against the reference's
rasters (tests/golden/distup_*.npz: every -m combination, -nc, -wg, -thresh), and against the C restatement of tests/distup_model.py (held
to those goldens by tests/test_distup_restatement.py) at sizes and cell geometries the goldens do not cover: nodata holes, ragged shapes
around the 64-cell tile, per-row `wild` cell sizes, both tile geometries under the sweep verifier, and three strips."""
import os
import subprocess

import numpy as np
import pytest

import distup_model as M
import taudem_amd as T
from cellsizes import rows
from conftest import bits_equal, describe_diff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")
MODES = [(s, k) for s in M.STATS for k in M.KINDS]


def same(a, b, name):
    assert bits_equal(a, b), describe_diff(a, b, name)


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("distup"))


def _inputs(ctx, oracle, shape, seed, dx=30.0, dy=30.0, holes=False):
    """(ang, fel, weights): angles of a pit-filled synthetic DEM, a few nodata elevations under valid angles, a few negative and a few
    nodata weights; with `holes` nodata blocks in the DEM."""
    rng = np.random.default_rng(seed)
    dem = oracle.synth_dem(shape, seed)
    ny, nx = shape
    if holes and ny > 8 and nx > 8:
        for _ in range(max(1, ny * nx // 40000)):
            y, x = rng.integers(0, ny - 4), rng.integers(0, nx - 4)
            dem[y:y + rng.integers(2, 12), x:x + rng.integers(2, 12)] = -9999.0
    fel = ctx.pitremove(dem, -9999.0)
    ang, _ = ctx.dinfflowdir(fel, -3.0e38, dx, dy)
    fel = fel.copy()
    fel[rng.random(shape) < 0.002] = -3.0e38
    w = (0.5 + rng.random(shape, dtype=np.float32) * 2.0).astype(np.float32)
    neg = rng.random(shape) < 0.02
    w[neg] = -w[neg]
    w[rng.random(shape) < 0.005] = -9999.0
    return ang, fel, w


def _check(ctx, restate, ang, fel, w, dx, dy, modes, what):
    for stat, kind in modes:
        for weights, cc, th, tag in ((None, True, 0.0, ""), (None, False, 0.0, " -nc"), (w, True, 0.0, " -wg"), (w, False, 0.3, " -wg -nc -thresh 0.3")):
            out = ctx.dinfdistup(ang, fel, stat=stat, kind=kind, weights=weights, contcheck=cc, thresh=th, dx=dx, dy=dy)
            ref = restate(ang, fel, stat=stat, kind=kind, weights=weights, contcheck=cc, thresh=th, dxc=dx, dyc=dy)
            same(out, ref, f"{stat} {kind}{tag}, {what}")


@pytest.mark.parametrize("name", M.golden_names())
@pytest.mark.parametrize("kind", list(M.KINDS))
def test_context_matches_reference_goldens(ctx, name, kind):
    g = M.load_golden(name)
    for stat, k, sfx in M.variants():
        if k != kind:
            continue
        out = ctx.dinfdistup(g["ang"], g["fel"], stat=stat, kind=kind, weights=g["wg"] if sfx == "_wg" else None, contcheck=sfx != "_nc",
                             thresh=M.THRESH if sfx == "_t" else 0.0, dx=g["dxc"], dy=g["dyc"])
        same(out, g[f"du_{stat}_{kind}{sfx}"], f"{name}: {stat} {kind}{sfx}")


def test_h_needs_no_fel_and_device_tensors(ctx):
    import torch

    g = M.load_golden("holes")
    out = ctx.dinfdistup(g["ang"], None, stat="max", kind="h", dx=g["dxc"], dy=g["dyc"])
    same(out, g["du_max_h"], "max h without fel")
    dev = f"cuda:{ctx.device}"
    ang, fel, wg = (torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in ("ang", "fel", "wg"))
    out = ctx.dinfdistup(ang, None, stat="ave", kind="h", thresh=M.THRESH, dx=g["dxc"], dy=g["dyc"])
    same(out.cpu().numpy(), g["du_ave_h_t"], "ave h -thresh on device tensors, without fel")
    out = ctx.dinfdistup(ang, fel, stat="ave", kind="p", weights=wg, dx=g["dxc"], dy=g["dyc"])
    same(out.cpu().numpy(), g["du_ave_p_wg"], "ave p -wg on device tensors")
    with pytest.raises(ValueError):
        ctx.dinfdistup(g["ang"], None, kind="v")


def test_restatement_1100x900_with_holes(ctx, oracle, restate):
    ang, fel, w = _inputs(ctx, oracle, (1100, 900), 17, holes=True)
    _check(ctx, restate, ang, fel, w, 30.0, 30.0, MODES, "1100 x 900 with holes")


@pytest.mark.parametrize("shape", [(1, 1), (1, 97), (97, 1), (63, 63), (64, 64), (65, 65), (63, 65), (65, 64), (64, 129), (130, 63)])
def test_restatement_ragged_shapes(ctx, oracle, restate, shape):
    ang, fel, w = _inputs(ctx, oracle, shape, 5 + shape[0] * 7 + shape[1])
    _check(ctx, restate, ang, fel, w, 10.0, 12.5, MODES, f"{shape[0]} x {shape[1]}")


@pytest.mark.parametrize("shape", [(257, 301), (65, 64), (700, 96)])
def test_restatement_wild_cell_sizes(ctx, oracle, restate, shape):
    dx, dy = rows("wild", shape[0], seed=shape[1])
    ang, fel, w = _inputs(ctx, oracle, shape, 23 + shape[1], dx=dx, dy=dy)
    _check(ctx, restate, ang, fel, w, dx, dy, MODES, f"{shape[0]} x {shape[1]} wild rows")


@pytest.mark.slow
def test_large_under_the_sweep_verifier(ctx, oracle, restate, monkeypatch):
    """3100 x 2900: the bulk rounds on 32 x 32 tiles hand over to 64 x 64 tiles, and TDX_SWEEP_VERIFY=1 re-evaluates every swept cell
    from its contributors' final records with the policy's own expression (both sweeps of p)."""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    ang, fel, w = _inputs(ctx, oracle, (3100, 2900), 31, holes=True)
    for stat, kind, weights, th in (("ave", "h", None, 0.0), ("max", "h", w, 0.0), ("min", "v", None, 0.3), ("max", "p", w, 0.0), ("ave", "s", None, 0.0)):
        out = ctx.dinfdistup(ang, fel, stat=stat, kind=kind, weights=weights, thresh=th, dx=30.0, dy=30.0)
        ref = restate(ang, fel, stat=stat, kind=kind, weights=weights, thresh=th, dxc=30.0, dyc=30.0)
        same(out, ref, f"{stat} {kind}{' -wg' if weights is not None else ''} -thresh {th}, 3100 x 2900")


def _run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([os.path.join(BIN, "dinfdistup"), *args], capture_output=True, text=True, timeout=120, env=e)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("name", M.golden_names())
@pytest.mark.parametrize("ngpus", [1, 3])
def test_cli_matches_reference_goldens(tmp_path, name, ngpus):
    g = M.load_golden(name)
    c = np.load(os.path.join(ROOT, "tests", "golden", f"case_{name}.npz"))
    ny = g["ang"].shape[0]
    dx, dy, geo = float(c["dx"]), float(c["dy"]), bool(c["geographic"])
    gt = (-111.9, dx, 0.0, 41.9, 0.0, -dy) if geo else (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)   # tests/golden/make_golden_distup.py
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("bang.tif"), g["ang"], -3.402823466e38, geotransform=gt, geographic=geo)   # the simple form's names: nameadd("b.tif", suffix)
    T.write_raster(f("bfel.tif"), g["fel"], -3.0e38, geotransform=gt, geographic=geo)
    T.write_raster(f("bwg.tif"), g["wg"], -9999.0, geotransform=gt, geographic=geo)
    N = ["--gpus", str(ngpus)]
    base = ["-ang", f("bang.tif"), "-fel", f("bfel.tif"), "-slp", f("never_read.tif")]
    out = _run(*N, *base, "-du", f("first.tif"), "-m", "ave", "v")
    assert "DinfDistUp -v version" in out and f"Processors: {ngpus}" in out
    runs = [(s, k, "") for s, k in MODES] + [("max", "s", "_nc"), ("ave", "h", "_nc"), ("min", "p", "_wg"), ("ave", "s", "_wg")]
    runs += [(s, k, "_t") for s, k in M.THRESH_RUNS]
    for i, (stat, kind, sfx) in enumerate(runs):
        extra = {"": [], "_nc": ["-nc"], "_wg": ["-wg", f("bwg.tif")], "_t": ["-thresh", str(M.THRESH)]}[sfx]
        order = [stat, kind] if i % 2 else [kind, stat]   # -m takes its two tokens in either order
        _run(*N, *base, *extra, "-du", f("du.tif"), "-m", *order)
        a, _ = T.read_raster(f("du.tif"), np.float32)
        same(a, g[f"du_{stat}_{kind}{sfx}"], f"{name}: -m {' '.join(order)} {' '.join(extra)} --gpus {ngpus}")
    _run(*N, f("b.tif"))   # simple form: nameadd suffixes ang fel slp wg du, no weights, default -m ave h
    a, _ = T.read_raster(f("bdu.tif"), np.float32)
    same(a, g["du_ave_h"], f"{name}: simple form --gpus {ngpus}")


@pytest.mark.slow
def test_three_strips_equal_one_gpu(ctx, oracle):
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows, strip_rows

    ny, nx = 3100, 2900
    dx, dy = rows("wild", ny, seed=3)
    ang, fel, w = _inputs(ctx, oracle, (ny, nx), 41, dx=dx, dy=dy, holes=True)
    modes = (("ave", "v", None, 0.0), ("max", "h", w, 0.0), ("min", "p", w, 0.3), ("ave", "s", None, 0.0))
    one = [ctx.dinfdistup(ang, fel, stat=s, kind=k, weights=wt, thresh=th, dx=dx, dy=dy) for s, k, wt, th in modes]
    parts = partition_rows(ny, 3)
    ts = {k: torch.from_numpy(v) for k, v in (("ang", ang), ("fel", fel), ("w", w))}
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
            res = []
            for s_, k_, wt, th in modes:
                du, _ = pipe.dinfdistup(loc["ang"], loc["fel"], stat=s_, kind=k_, weights=loc["w"] if wt is not None else None, thresh=th, dx=sdx, dy=sdy)
                torch.cuda.synchronize()
                res.append(du[1:y1 - y0 + 1].cpu().numpy())
            return res
        res = grp.run(rank_main)
    for i, (s, k, wt, th) in enumerate(modes):
        same(np.concatenate([r[i] for r in res]), one[i], f"{s} {k}{' -wg' if wt is not None else ''} -thresh {th} in three strips")
