"""MoveOutletsToStrm and ConnectDown on the GPU (taudem_amd/csrc/outlettools.hip): Context.moveoutletstostrm / Context.connectdown and the two
command-line tools against the real tools' recorded outputs (tests/golden/outlets_*.npz: the five cases and the hand-built rasters, -md 50 / 3 and
-d 10 / 2) - coordinates to the bit, fields as text - and against the C restatement of tests/outlets_model.py (held to those goldens by
tests/test_outlets_restatement.py) where no golden reaches: generated rasters with a few hundred outlets, and the arg-max by itself on widths
around the 8 cells of a lane, runs of equal id that end on a lane, a wave and a workgroup boundary, ids up to the largest one supported, and the
refusals.  The cases are 100 x 120 and the like: several workgroups of 2048 cells, rows that are no multiple of a lane's 8 cells."""
import os
import subprocess

import numpy as np
import pytest

import outlets_model as M
import taudem_amd as T
import vector_parse as V
from taudem_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("outlets"))


def case_inputs(name):
    p, src, w, ad8, gt, geographic = M.inputs(name)
    g = M.load_golden(name)
    return g, dict(p=p, src=src, w=w, ad8=ad8, gt=gt, geographic=geographic, ox=g["ox"], oy=g["oy"], ids=g["ids"])


def small_inputs(name):
    g = M.load_golden("small")
    p, w, ad8 = M.small_rasters()[name]
    return g, dict(p=p, src=M.small_src(w, ad8), w=w, ad8=ad8, gt=M.SMALL_GT, geographic=False, ox=g[name + "_ox"], oy=g[name + "_oy"], ids=g[name + "_ids"])


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def move_context(ctx, i, md, device=False):
    cols, rows = M.to_cells(i["gt"], i["ox"], i["oy"])
    f = dev if device else (lambda a: a)
    rx, ry, d = ctx.moveoutletstostrm(f(i["p"]), f(i["src"]), (cols, rows), md, src_nodata=M.SRC_NODATA)
    assert all(isinstance(a, np.ndarray) and a.dtype == np.int32 for a in (rx, ry, d))
    return M.move_record(i["gt"], i["ox"], i["oy"], i["ids"], rx, ry, d)


def connect_context(ctx, i, dd, device=False):
    f = dev if device else (lambda a: a)
    res = ctx.connectdown(f(i["p"]), f(i["w"]), f(i["ad8"]), dd)
    assert all(isinstance(a, np.ndarray) for a in res) and res[3].dtype == np.float32
    return res


def assert_context_equals_golden(ctx, g, i, tag, prefix=""):
    for md in M.MAXDISTS:
        want = bytes(g[f"{prefix}move_md{md}"])
        assert move_context(ctx, i, md) == want, f"{tag}: -md {md}"
        assert move_context(ctx, i, md, device=True) == want, f"{tag}: -md {md}, device form"
    for dd in M.MOVEDISTS:
        host, devres = connect_context(ctx, i, dd), connect_context(ctx, i, dd, device=True)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(host, devres)), f"{tag}: -d {dd}: host and device forms differ"
        if prefix and int(g[prefix + "nopoints"]):
            assert host[0].size == 0
            continue
        o, od = M.connect_records(i["gt"], host)
        assert o == bytes(g[f"{prefix}connect_o_d{dd}"]) and od == bytes(g[f"{prefix}connect_od_d{dd}"]), f"{tag}: -d {dd}"


@pytest.mark.parametrize("name", M.CASES)
def test_context_matches_reference_cases(ctx, name):
    g, i = case_inputs(name)
    assert_context_equals_golden(ctx, g, i, name)


@pytest.mark.parametrize("name", sorted(M.small_rasters()))
def test_context_matches_reference_hand_built(ctx, name):
    g, i = small_inputs(name)
    assert_context_equals_golden(ctx, g, i, name, name + "_")


# ---- the command-line tools ----------------------------------------------------------------------------------------------------------------
def write_inputs(tmp_path, i):
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("p.tif"), i["p"], M.P_NODATA, geotransform=i["gt"], geographic=i["geographic"])
    T.write_raster(f("src.tif"), i["src"].astype(np.int16), M.SRC_NODATA, geotransform=i["gt"], geographic=i["geographic"])
    T.write_raster(f("w.tif"), i["w"], M.W_NODATA, geotransform=i["gt"], geographic=i["geographic"])
    T.write_raster(f("ad8.tif"), i["ad8"], M.AD8_NODATA, geotransform=i["gt"], geographic=i["geographic"])
    with open(f("outlets.txt"), "w") as fo:
        for x, y, k in zip(i["ox"], i["oy"], i["ids"]):
            fo.write(f"{float(x)!r} {float(y)!r} {int(k)}\n")
    return f


def run_move(f, out, md, gpus=None):
    args = [os.path.join(BIN, "moveoutletstostrm")] + (["--gpus", str(gpus)] if gpus else []) + ["-p", f("p.tif"), "-src", f("src.tif"), "-o", f("outlets.txt"), "-om", f(out),
                                                                                                   "-md", str(md)]
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def run_connect(f, o, od, dd, gpus=None, check=True):
    args = [os.path.join(BIN, "connectdown")] + (["--gpus", str(gpus)] if gpus else []) + ["-p", f("p.tif"), "-w", f("w.tif"), "-ad8", f("ad8.tif"), "-o", f(o), "-od", f(od),
                                                                                             "-d", str(dd)]
    r = subprocess.run(args, capture_output=True, text=True)
    assert not check or r.returncode == 0, r.stdout + r.stderr
    return r


def layer_record(path, real=()):
    """The record lines of a written layer.  GeoJSON holds every number with 17 digits; a .dbf column holds a Real with 15 decimals, so `real`
    fields of a shapefile are taken through float32 (what ad8 is) before they are written out again."""
    if path.endswith(".shp"):
        pts = V.shapefile_points(path)
        fmt = lambda k, v: M._num(np.float64(np.float32(float(v)))) if k in real else v  # noqa: E731
    else:
        pts = V.geojson(path)[0]
        fmt = lambda k, v: M._num(v) if k in real else ("" if v is None else str(v))  # noqa: E731
    return "".join(f"{M._num(x)} {M._num(y)} " + " ".join(f"{k}={fmt(k, v)}" for k, v in props.items()) + "\n" for x, y, props in pts).encode()


def assert_cli_equals_golden(tmp_path, g, i, tag, prefix="", gpus=None):
    f = write_inputs(tmp_path, i)
    for md, ext in zip(M.MAXDISTS, (".shp", ".geojson")):
        r = run_move(f, f"moved{md}{ext}", md, gpus)
        assert r.stdout.startswith("MoveOutletsToStreams version ") and "Total time: " in r.stdout
        assert layer_record(f(f"moved{md}{ext}")) == bytes(g[f"{prefix}move_md{md}"]), f"{tag}: -md {md} {ext}"
    for dd, (eo, eod) in zip(M.MOVEDISTS, ((".geojson", ".shp"), (".shp", ".json"))):
        r = run_connect(f, f"o{dd}{eo}", f"od{dd}{eod}", dd, gpus)
        assert r.stdout.startswith("ConnectDown version ")
        if prefix and int(g[prefix + "nopoints"]):
            assert "No points found\n\n" in r.stdout and not os.path.exists(f(f"o{dd}{eo}")) and not os.path.exists(f(f"od{dd}{eod}"))
            continue
        finite = b"nan" not in bytes(g[f"{prefix}connect_o_d{dd}"])
        for path, key in ((f"o{dd}{eo}", "connect_o_d"), (f"od{dd}{eod}", "connect_od_d")):
            if path.endswith(".shp") or finite:       # (GeoJSON has no NaN: such an ad8 is written as null)
                assert layer_record(f(path), real=("ad8",)) == bytes(g[f"{prefix}{key}{dd}"]), f"{tag}: -d {dd} {path}"


@pytest.mark.parametrize("name", M.CASES)
def test_cli_matches_reference_cases(tmp_path, name):
    g, i = case_inputs(name)
    assert_cli_equals_golden(tmp_path, g, i, name)


@pytest.mark.parametrize("name", sorted(M.small_rasters()))
def test_cli_matches_reference_hand_built(tmp_path, name):
    g, i = small_inputs(name)
    assert_cli_equals_golden(tmp_path, g, i, name, name + "_")


# ---- generated rasters against the restatement ---------------------------------------------------------------------------------------------
def generated(ctx, oracle, shape, seed):
    from test_gpu_streamnet import generated as streamnet_inputs

    i = streamnet_inputs(ctx, oracle, shape, seed)
    _, w, _, _ = ctx.streamnet(i["p"], i["src"], i["fel"], i["ad8"], dx=i["dx"], dy=i["dy"], geotransform=i["gt"])
    rng = np.random.default_rng(seed + 5)
    ny, nx = shape
    n = 400
    cols, rows = rng.integers(-2, nx + 2, n).astype(np.int32), rng.integers(-2, ny + 2, n).astype(np.int32)
    return dict(p=i["p"], src=i["src"], w=w, ad8=i["ad8"], cols=cols, rows=rows)


@pytest.mark.parametrize("shape", [(65, 129), (130, 150)])
def test_generated_rasters_equal_the_restatement(ctx, oracle, restate, shape):
    i = generated(ctx, oracle, shape, 11 + shape[0])
    for md in (50, 7, 0):
        want = restate.moveoutlets(i["p"], i["src"], i["cols"], i["rows"], md)
        for f in (lambda a: a, dev):
            got = ctx.moveoutletstostrm(f(i["p"]), f(i["src"]), (i["cols"], i["rows"]), md, src_nodata=M.SRC_NODATA)
            assert all(np.array_equal(a, b) for a, b in zip(want, got)), f"{shape} -md {md}"
        assert md != 50 or ((want[2] > 0).sum() > 30 and (want[2] == -1).sum() > 5)
    for dd in (10, 1, 0):
        want = restate.connectdown(i["p"], i["w"], i["ad8"], dd)
        for f in (lambda a: a, dev):
            got = ctx.connectdown(f(i["p"]), f(i["w"]), f(i["ad8"]), dd)
            assert len(want[0]) > 5 and all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(want, got)), f"{shape} -d {dd}"


# ---- the arg-max by itself (movedist 0) ------------------------------------------------------------------------------------------------------
def argmax_equals(ctx, restate, w, ad8, tag):
    p = np.full(w.shape, 1, np.int16)
    want = restate.connectdown(p, w, ad8, 0)
    got = ctx.connectdown(p, np.ascontiguousarray(w, np.int32), np.ascontiguousarray(ad8, np.float32), 0)
    for a, b, what in zip(want, got, ("ids", "columns", "rows", "ad8max", "moved columns", "moved rows", "id_down")):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{tag}: {what} differ"
    return got


@pytest.mark.parametrize("nx", [1, 7, 8, 9, 255, 257])
def test_argmax_on_widths_around_a_lane(ctx, restate, nx):
    rng = np.random.default_rng(nx)
    ny = 37
    w = rng.integers(0, 9, (ny, nx)).astype(np.int32)
    w[rng.random((ny, nx)) < 0.1] = M.W_NODATA
    ad8 = rng.integers(0, 6, (ny, nx)).astype(np.float32)            # few values: ties everywhere
    ad8[rng.random((ny, nx)) < 0.02] = np.nan
    ad8[rng.random((ny, nx)) < 0.02] = -0.0
    argmax_equals(ctx, restate, w, ad8, f"nx {nx}")
    blocks = np.repeat(np.repeat(rng.integers(0, 5, ((ny + 5) // 6, (nx + 10) // 11)), 6, axis=0), 11, axis=1)[:ny, :nx].astype(np.int32)   # coherent labels
    argmax_equals(ctx, restate, blocks, ad8, f"nx {nx}, blocks")


@pytest.mark.parametrize("boundary", [8, 64 * 8, 256 * 8])
def test_argmax_runs_that_end_on_a_boundary(ctx, restate, boundary):
    """runs of equal id that end exactly where a lane's 8 cells, a wave's 512 and a workgroup's 2048 end, with the maximum on either side of it"""
    n = 3 * 2048 + 5
    for shift in (0, 1):
        w = np.full((1, n), 3, np.int32)
        w[0, boundary + shift:] = 4
        w[0, 2 * boundary:] = 3
        ad8 = np.ones((1, n), np.float32)
        for at in (boundary - 1, boundary, boundary + 1, 2 * boundary - 1, 2 * boundary):
            ad8[0, at] = 7
        argmax_equals(ctx, restate, w, ad8, f"boundary {boundary} shift {shift}")
        ad8[0, boundary - 1] = 9
        got = argmax_equals(ctx, restate, w, ad8, f"boundary {boundary} shift {shift}, maximum on the last cell before it")
        assert list(got[0]) == [3, 4] and got[1][0] == boundary - 1


def test_argmax_checkerboard_and_large_ids(ctx, restate):
    yy, xx = np.mgrid[0:70, 0:130]
    w = ((yy + xx) % 2 + 1).astype(np.int32)
    ad8 = ((yy * 7 + xx * 13) % 31).astype(np.float32)
    argmax_equals(ctx, restate, w, ad8, "checkerboard")
    w = ((yy * 130 + xx) % 5000 * 3).astype(np.int32)                   # one atomic per cell into 5000 ids
    argmax_equals(ctx, restate, w, ad8, "one id per cell")
    w = np.full((3, 5), M.W_NODATA, np.int32)
    w[0, 1] = w[2, 2] = _lib.CONNECTDOWN_MAX_ID
    w[1, 1] = 0
    ad8 = np.arange(15, dtype=np.float32).reshape(3, 5)
    p = np.full((3, 5), 1, np.int16)
    ids, x, y, amax, *_ = ctx.connectdown(p, w, ad8, 0)
    assert list(ids) == [0, _lib.CONNECTDOWN_MAX_ID] and (x[1], y[1], amax[1]) == (2, 2, 12.0)
    assert _lib.CONNECTDOWN_MAX_ID == M.MAX_ID


def test_refusals(ctx, tmp_path):
    p = np.full((3, 5), 1, np.int16)
    ad8 = np.ones((3, 5), np.float32)
    for bad, word in ((-1, "negative"), (_lib.CONNECTDOWN_MAX_ID + 1, "above")):
        w = np.full((3, 5), 2, np.int32)
        w[2, 4] = bad
        with pytest.raises(_lib.TdxError) as e:
            ctx.connectdown(p, w, ad8, 2)
        assert e.value.code == _lib.TDX_ERR_ARG and word in str(e.value) and str(bad) in str(e.value)
    assert ctx.connectdown(p, np.full((3, 5), 2, np.int32), ad8, 2)[0].tolist() == [2]   # the context works on
    i = dict(p=p, src=np.zeros((3, 5), np.int32), w=w, ad8=ad8, gt=M.SMALL_GT, geographic=False, ox=[205.0], oy=[890.0], ids=[1])
    f = write_inputs(tmp_path, i)
    r = run_connect(f, "o.shp", "od.shp", 2, check=False)
    assert r.returncode == 2 and "above" in r.stderr and not os.path.exists(f("o.shp")) and not os.path.exists(f("od.shp"))
