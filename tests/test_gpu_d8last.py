"""FlowDirCond, D8VDistToStrm and SlopeAveDown on the GPU (taudem_amd/csrc/flowdircond.hip, d8rev.hip, slopeavedown.hip): Context.flowdircond /
.d8vdisttostrm / .slopeavedown, the StripPipeline methods and the three command-line tools against the reference's outputs
(tests/golden/d8last_*.npz) and against the C restatement of tests/d8last_model.py (held to those goldens by
tests/test_d8last_restatement.py) at sizes and cell geometries the goldens do not cover: ragged shapes around the tile edges, one row, one
column, per-row cell sizes, nodata holes, 2048 x 2176, both tile geometries under the sweep verifier, three strips whose cut rows long flow
paths cross, SlopeAveDown with more passes than a strip is tall, device tensors.  Bit for bit everywhere, no cell left out."""
import os
import subprocess

import numpy as np
import pytest

import d8last_model as M
import taudem_amd as T
from cellsizes import rows
from conftest import bits_equal, describe_diff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")
SRC_ND = -2147483647
FEL_ND = M.FEL_NODATA
CASES = ("fourway_mask", "geographic", "holes", "plain", "rect_dxdy")


def same(a, b, name):
    assert bits_equal(a, b), describe_diff(a, b, name)


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("d8last"))


def _inputs(ctx, oracle, shape, seed, dx=30.0, dy=30.0, holes=False):
    """(p, src, fel, z): D8 directions of a pit-filled synthetic DEM with a few p == 0 cells; src = 1 on the top 6 % of AreaD8 with nodata holes
    (int32, nodata SRC_ND); fel with nodata planted under valid directions; z = fel + seeded noise of 3 m (not pit-filled along p)."""
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
    fel = np.where(fel < -1e30, np.float32(FEL_ND), fel).astype(np.float32)
    fel[(rng.random(shape) < 0.003) & (p >= 1)] = FEL_ND
    z = fel.copy()
    ok = z > -1e30
    z[ok] = (z[ok] + rng.normal(0.0, 3.0, int(ok.sum()))).astype(np.float32)
    return p, src, fel, z


def _check(ctx, restate, p, src, fel, z, dx, dy, what, factors=M.DN_FACTORS):
    same(ctx.flowdircond(p, z, z_nodata=FEL_ND), restate.flowdircond(p, z, FEL_ND), f"zfdc, {what}")
    same(ctx.d8vdisttostrm(p, fel, src, 1, src_nodata=SRC_ND), restate.vdist(p, fel, src, 1, src_nodata=SRC_ND), f"vdist, {what}")
    dxc, dyc = np.broadcast_to(np.asarray(dx, np.float64), (p.shape[0],)), np.broadcast_to(np.asarray(dy, np.float64), (p.shape[0],))
    m = min(abs(float(dxc[p.shape[0] // 2])), abs(float(dyc[p.shape[0] // 2])))
    for fct in factors:
        dn = fct * m
        same(ctx.slopeavedown(p, fel, dn, dx=dx, dy=dy, fel_nodata=FEL_ND), restate.slopeavedown(p, fel, dn, dx, dy, FEL_ND), f"slpd dn {dn}, {what}")


@pytest.mark.parametrize("name", CASES)
def test_context_matches_reference_goldens(ctx, name):
    g = M.load_golden(name)
    nd = float(g["fel_nodata"])
    same(ctx.flowdircond(g["p"], g["z"], z_nodata=nd), g["zfdc"], f"{name}: zfdc")
    same(ctx.d8vdisttostrm(g["p"], g["fel"], g["src"], src_nodata=int(g["src_nodata"])), g["vdist_src"], f"{name}: -src src")
    same(ctx.d8vdisttostrm(g["p"], g["fel"], g["ad8"], M.THRESH_AD8, src_nodata=int(g["ad8_nodata"])), g["vdist_ad8"], f"{name}: -src ad8 -thresh {M.THRESH_AD8}")
    for i in range(3):
        out, st = ctx.slopeavedown(g["p"], g["fel"], float(g["dn"][i]), dx=g["dxc"], dy=g["dyc"], fel_nodata=nd, stats=True)
        assert st["rounds"] == int(g["niter"][i])
        same(out, g[f"slpd_{i}"], f"{name}: -dn {float(g['dn'][i])}")


def test_device_tensors(ctx):
    import torch

    g = M.load_golden("holes")
    dev = f"cuda:{ctx.device}"
    p, src, fel, z = (torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in ("p", "src", "fel", "z"))
    nd = float(g["fel_nodata"])
    out = ctx.flowdircond(p, z, z_nodata=nd)
    assert out.is_cuda
    same(out.cpu().numpy(), g["zfdc"], "device tensors: zfdc")
    same(z.cpu().numpy(), g["z"], "device tensors: z is not written")
    out = ctx.d8vdisttostrm(p, fel, src, src_nodata=int(g["src_nodata"]))
    assert out.is_cuda
    same(out.cpu().numpy(), g["vdist_src"], "device tensors: vdist")
    out = ctx.slopeavedown(p, fel, float(g["dn"][2]), dx=g["dxc"], dy=g["dyc"], fel_nodata=nd)
    assert out.is_cuda
    same(out.cpu().numpy(), g["slpd_2"], "device tensors: slpd")


@pytest.mark.parametrize("shape", [(1, 1), (1, 97), (97, 1), (31, 33), (32, 32), (33, 31), (63, 63), (64, 64), (65, 65), (63, 65), (64, 129), (130, 63), (3, 257), (257, 3)])
def test_restatement_ragged_shapes(ctx, oracle, restate, shape):
    p, src, fel, z = _inputs(ctx, oracle, shape, 5 + shape[0] * 7 + shape[1])
    _check(ctx, restate, p, src, fel, z, 10.0, 12.5, f"{shape[0]} x {shape[1]}")


@pytest.mark.parametrize("kind,shape", [("wild", (257, 301)), ("wild", (65, 64)), ("band", (700, 96)), ("fine", (300, 200))])
def test_restatement_per_row_cell_sizes(ctx, oracle, restate, kind, shape):
    dx, dy = rows(kind, shape[0], seed=shape[1])
    p, src, fel, z = _inputs(ctx, oracle, shape, 23 + shape[1], dx=dx, dy=dy)
    _check(ctx, restate, p, src, fel, z, dx, dy, f"{shape[0]} x {shape[1]} {kind} rows")


def test_restatement_2048_with_holes(ctx, oracle, restate):
    p, src, fel, z = _inputs(ctx, oracle, (2048, 2176), 17, holes=True)
    _check(ctx, restate, p, src, fel, z, 30.0, 30.0, "2048 x 2176 with holes", factors=(0.5, 6.2, 40.3))


def test_sweep_tools_under_the_sweep_verifier(ctx, oracle, restate, monkeypatch):
    """3100 x 2900: the bulk rounds on 32 x 32 tiles hand over to 64 x 64 tiles, and TDX_SWEEP_VERIFY=1 re-evaluates every swept cell from
    its contributors' (FlowDirCond, SlopeAveDown's popped set) or its receiver's (D8VDistToStrm) final records."""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    p, src, fel, z = _inputs(ctx, oracle, (3100, 2900), 31, holes=True)
    _check(ctx, restate, p, src, fel, z, 30.0, 30.0, "3100 x 2900 under the verifier", factors=(2.5,))


def test_small_tiles_only_under_the_sweep_verifier(ctx, oracle, restate, monkeypatch):
    """700 x 900 with TDX_D8_BULK_UNTIL=1: every round but the last few runs on 32 x 32 tiles."""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    p, src, fel, z = _inputs(ctx, oracle, (700, 900), 77, holes=True)
    _check(ctx, restate, p, src, fel, z, 30.0, 30.0, "700 x 900 under the verifier", factors=(2.5,))


def _three_strips(ny, nx, arrays, body):
    """Runs body(pipe, local arrays, y0, y1) on three ranks; returns the per-rank results."""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows

    parts = partition_rows(ny, 3)
    ts = {k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in arrays.items()}
    with StripGroup(3, nx) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            pipe = StripPipeline(c, comm, nx, y1 - y0)
            loc = {}
            for k, t in ts.items():
                s = pipe.empty(t.dtype)
                s[1:y1 - y0 + 1].copy_(t[y0:y1])
                loc[k] = s
            outs = body(pipe, loc, y0, y1)
            torch.cuda.synchronize()
            return [o[1:y1 - y0 + 1].cpu().numpy() for o in outs]
        return grp.run(rank_main)


def test_three_strips_equal_restatement(ctx, oracle, restate):
    from taudem_amd.distributed import strip_rows

    ny, nx = 1500, 1300
    dx, dy = rows("wild", ny, seed=3)
    p, src, fel, z = _inputs(ctx, oracle, (ny, nx), 41, dx=dx, dy=dy, holes=True)
    dn = 12.3 * min(abs(float(dx[ny // 2])), abs(float(dy[ny // 2])))
    niter = M.niter_of(dn, dx, dy)
    assert niter == 13

    def body(pipe, loc, y0, y1):
        zfdc, _ = pipe.flowdircond(loc["p"], loc["z"], z_nodata=FEL_ND)
        vd, _ = pipe.d8vdisttostrm(loc["p"], loc["fel"], loc["src"], 1, src_nodata=SRC_ND)
        sd, _ = pipe.slopeavedown(loc["p"], loc["fel"], dn, niter, dx=strip_rows(dx, y0, y1), dy=strip_rows(dy, y0, y1), fel_nodata=FEL_ND)
        return zfdc, vd, sd

    res = _three_strips(ny, nx, {"p": p, "src": src, "fel": fel, "z": z}, body)
    ref = (restate.flowdircond(p, z, FEL_ND), restate.vdist(p, fel, src, 1, src_nodata=SRC_ND), restate.slopeavedown(p, fel, dn, dx, dy, FEL_ND))
    # the cut rows are crossed by flow paths: cells on both sides of every cut have receivers on the other side
    for cut in (ny // 3, 2 * (ny // 3)):
        assert np.any(np.isin(p[cut - 1], (6, 7, 8))) and np.any(np.isin(p[cut], (2, 3, 4)))
    for i, what in enumerate(("zfdc", "vdist", "slpd")):
        same(np.concatenate([r[i] for r in res]), ref[i], f"{what} in three strips")


def test_slopeavedown_more_passes_than_a_strip_is_tall(ctx, oracle, restate):
    """Three strips of 20 rows, 45 passes: a record travels further than a strip is tall, through both cuts.  Only cells whose flow path is
    45 cells long get a slope on a raster 60 rows tall; the floor of 1 % (240 cells) keeps the comparison from being empty."""
    ny, nx = 60, 400
    p, src, fel, z = _inputs(ctx, oracle, (ny, nx), 59)
    dn = 44.5 * 30.0
    niter = M.niter_of(dn, 30.0, 30.0)
    assert niter == 45

    def body(pipe, loc, y0, y1):
        return (pipe.slopeavedown(loc["p"], loc["fel"], dn, niter, dx=30.0, dy=30.0, fel_nodata=FEL_ND)[0],)

    res = _three_strips(ny, nx, {"p": p, "fel": fel}, body)
    ref = restate.slopeavedown(p, fel, dn, 30.0, 30.0, FEL_ND)
    assert np.mean(ref != np.float32(-3.4028235e38)) > 0.01
    same(np.concatenate([r[0] for r in res]), ref, "slpd, 45 passes over strips of 20 rows")
    same(ctx.slopeavedown(p, fel, dn, dx=30.0, dy=30.0, fel_nodata=FEL_ND), ref, "slpd, 45 passes, one strip")


def _run(tool, *args, ok=True):
    r = subprocess.run([os.path.join(BIN, tool), *args], capture_output=True, text=True, timeout=180)
    if ok:
        assert r.returncode == 0, r.stdout + r.stderr
    return r


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("ngpus", [1, 3])
def test_cli_matches_context_and_goldens(ctx, tmp_path, name, ngpus):
    g = M.load_golden(name)
    gt, geo = tuple(float(v) for v in g["gt"]), bool(g["geographic"])
    nd = float(g["fel_nodata"])
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("bp.tif"), g["p"], M.P_NODATA, geotransform=gt, geographic=geo)   # the simple form's names: nameadd("b.tif", suffix)
    T.write_raster(f("bsrc.tif"), g["src"].astype(np.int16), int(g["src_nodata"]), geotransform=gt, geographic=geo)
    T.write_raster(f("ad8.tif"), g["ad8"], int(g["ad8_nodata"]), geotransform=gt, geographic=geo)
    T.write_raster(f("bfel.tif"), g["fel"], nd, geotransform=gt, geographic=geo)
    T.write_raster(f("bz.tif"), g["z"], nd, geotransform=gt, geographic=geo)
    info = T.read_raster(f("bfel.tif"), np.float32)[1]
    N = ["--gpus", str(ngpus)]

    def expect(path, arr, nodata, what):
        """The raster in the tool's file equals the Context result byte for byte, and carries the expected nodata value."""
        got, inf = T.read_raster(path, np.float32)
        assert got.tobytes() == np.ascontiguousarray(arr).tobytes(), what
        assert np.float32(inf["nodata"]) == np.float32(nodata), what

    out = _run("flowdircond", *N, "-p", f("bp.tif"), "-z", f("bz.tif"), "-zfdc", f("zfdc.tif")).stdout
    assert "FlowDirCond version" in out and f"Processors: {ngpus}" in out
    zfdc = ctx.flowdircond(g["p"], g["z"], z_nodata=nd)
    same(zfdc, g["zfdc"], f"{name}: Context zfdc")
    expect(f("zfdc.tif"), zfdc, nd, f"{name}: flowdircond --gpus {ngpus}")
    _run("flowdircond", *N, f("b.tif"))
    same(T.read_raster(f("bzfdc.tif"), np.float32)[0], g["zfdc"], f"{name}: flowdircond simple form --gpus {ngpus}")

    out = _run("d8vdisttostrm", *N, "-p", f("bp.tif"), "-fel", f("bfel.tif"), "-src", f("bsrc.tif"), "-dist", f("v1.tif")).stdout
    assert "D8VDistToStrm version" in out and f"Processors: {ngpus}" in out
    expect(f("v1.tif"), ctx.d8vdisttostrm(g["p"], g["fel"], g["src"], src_nodata=int(g["src_nodata"])), -3.402823466e38, f"{name}: d8vdisttostrm --gpus {ngpus}")
    same(T.read_raster(f("v1.tif"), np.float32)[0], g["vdist_src"], f"{name}: d8vdisttostrm --gpus {ngpus} against the golden")
    _run("d8vdisttostrm", *N, "-p", f("bp.tif"), "-fel", f("bfel.tif"), "-src", f("ad8.tif"), "-thresh", str(M.THRESH_AD8), "-dist", f("v2.tif"))
    same(T.read_raster(f("v2.tif"), np.float32)[0], g["vdist_ad8"], f"{name}: d8vdisttostrm -thresh --gpus {ngpus}")
    _run("d8vdisttostrm", *N, f("b.tif"))
    same(T.read_raster(f("bdist.tif"), np.float32)[0], g["vdist_src"], f"{name}: d8vdisttostrm simple form --gpus {ngpus}")

    for i in range(3):
        dn = float(g["dn"][i])
        r = _run("slopeavedown", *N, "-p", f("bp.tif"), "-fel", f("bfel.tif"), "-slpd", f(f"s{i}.tif"), "-dn", repr(dn))
        assert "SlopeAveDown version" in r.stdout and f"Processors: {ngpus}" in r.stdout and f"interations to do {int(g['niter'][i])}" in r.stderr
        expect(f(f"s{i}.tif"), ctx.slopeavedown(g["p"], g["fel"], dn, dx=info["dxc"], dy=info["dyc"], fel_nodata=nd), -3.402823466e38,
               f"{name}: slopeavedown -dn {dn} --gpus {ngpus}")
        same(T.read_raster(f(f"s{i}.tif"), np.float32)[0], g[f"slpd_{i}"], f"{name}: slopeavedown -dn {dn} --gpus {ngpus} against the golden")
    _run("slopeavedown", *N, f("b.tif"))   # simple form: -dn 50
    same(T.read_raster(f("bslpd.tif"), np.float32)[0], ctx.slopeavedown(g["p"], g["fel"], 50.0, dx=info["dxc"], dy=info["dyc"], fel_nodata=nd),
         f"{name}: slopeavedown simple form --gpus {ngpus}")


def test_cli_refusals(tmp_path):
    g = M.load_golden("plain")
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("p.tif"), g["p"], M.P_NODATA)
    T.write_raster(f("fel.tif"), g["fel"], float(g["fel_nodata"]))
    T.write_raster(f("src.tif"), g["src"].astype(np.int16), int(g["src_nodata"]))
    T.write_raster(f("small.tif"), g["fel"][:-3, :-5], float(g["fel_nodata"]))
    for bad in ("-5", "nan", "inf", "-inf", "12x"):
        r = _run("slopeavedown", "-p", f("p.tif"), "-fel", f("fel.tif"), "-slpd", f("s.tif"), "-dn", bad, ok=False)
        assert r.returncode != 0 and "-dn must be" in r.stderr, bad
        assert not os.path.exists(f("s.tif"))
    r = _run("slopeavedown", "-p", f("p.tif"), "-fel", f("small.tif"), "-slpd", f("s.tif"), ok=False)
    assert r.returncode != 0 and "File sizes do not match" in r.stdout and not os.path.exists(f("s.tif"))
    r = _run("flowdircond", "-p", f("p.tif"), "-z", f("small.tif"), "-zfdc", f("z.tif"), ok=False)
    assert r.returncode != 0 and "File sizes do not match" in r.stdout and not os.path.exists(f("z.tif"))
    r = _run("d8vdisttostrm", "-p", f("p.tif"), "-fel", f("small.tif"), "-src", f("src.tif"), "-dist", f("d.tif"), ok=False)
    assert r.returncode != 0 and "File sizes do not match" in r.stdout and not os.path.exists(f("d.tif"))
    from taudem_amd import tools

    assert tools.sloped(f("p.tif"), f("fel.tif"), f("s.tif"), dn=-1.0) != 0
    assert tools.sloped(f("p.tif"), f("fel.tif"), f("s.tif"), dn=float("nan")) != 0
    assert tools.flowdircond(f("p.tif"), f("small.tif"), f("z.tif")) != 0


def test_api_refuses_a_bad_dn(ctx):
    g = M.load_golden("plain")
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(Exception):
            ctx.slopeavedown(g["p"], g["fel"], bad, dx=g["dxc"], dy=g["dyc"])


def test_tools_module_matches_goldens(tmp_path):
    from taudem_amd import tools

    g = M.load_golden("rect_dxdy")
    gt, nd = tuple(float(v) for v in g["gt"]), float(g["fel_nodata"])
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("p.tif"), g["p"], M.P_NODATA, geotransform=gt)
    T.write_raster(f("src.tif"), g["src"].astype(np.int16), int(g["src_nodata"]), geotransform=gt)
    T.write_raster(f("fel.tif"), g["fel"], nd, geotransform=gt)
    T.write_raster(f("z.tif"), g["z"], nd, geotransform=gt)
    assert tools.flowdircond(f("p.tif"), f("z.tif"), f("zfdc.tif")) == 0
    same(T.read_raster(f("zfdc.tif"), np.float32)[0], g["zfdc"], "tools.flowdircond")
    assert tools.d8vdistdown(f("p.tif"), f("fel.tif"), f("src.tif"), f("v.tif")) == 0
    same(T.read_raster(f("v.tif"), np.float32)[0], g["vdist_src"], "tools.d8vdistdown")
    assert tools.sloped(f("p.tif"), f("fel.tif"), f("s.tif"), float(g["dn"][1])) == 0
    same(T.read_raster(f("s.tif"), np.float32)[0], g["slpd_1"], "tools.sloped")
