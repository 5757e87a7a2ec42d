"""Watershed polygons on the GPU (Context.polygonize, StripPipeline.polygonize_edges -> Polygons, bin/watershedgridtoshp) against the model
(tests/polygonize_model.py): ids, cells, the three offset lists and the vertices are equal exactly, and the edge columns are the model's.

Shapes that find kernel faults: 1 x 1, 1 x N, N x 1, 5 x 67 and 70 x 300 (more than one block of 2048 cells; neither size a multiple of the 8 cells of a
thread), 64 x 65 of two ids as a checkerboard (four edges per cell: the scan's worst case), diagonal stripes (every inner vertex a saddle), id 1 with a hole
of id 2 that holds an island of id 1, all nodata, one id, negative ids and 0, and the recorded w grids of StreamNet.  Every shape runs from a numpy array,
from a tensor that starts on a 16-byte boundary and from one that starts 4 bytes off it; widths that are multiples of 4 take the 16-byte loads in the
first two forms (68 x 12, 96 x 128, 64-wide cases), all others and every off-boundary tensor the cell-wide loads.

Strips: cut at 2, at 3 and with every row a strip of its own, with regions, saddles and holes on the cut rows; the merged result equals the one-device
result; the halo rows beyond the raster's top and bottom hold a poison id that changes nothing; no halo row is written."""
import os
import subprocess

import numpy as np
import pytest
import torch

import polygon_parse as P
import polygonize_model as M
import taudem_amd as T
from taudem_amd import api
from test_polygonize_model import HAND, RECORDED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "taudem_amd", "bin", "watershedgridtoshp")
ND = M.NODATA
POISON = 77777


def _grids():
    rng = np.random.default_rng(11)
    g = {k: HAND[k] for k in ("one_cell", "saddle", "ring_around_nodata", "nested", "all_nodata", "single_id", "negative_and_zero", "cut")}
    g["row_1x37"] = rng.integers(0, 3, (1, 37)).astype(np.int32)
    g["column_41x1"] = rng.integers(0, 3, (41, 1)).astype(np.int32)
    blobs = rng.integers(-2, 4, (5, 67)).astype(np.int32)
    blobs[blobs == 3] = ND
    g["random_5x67"] = blobs
    big = (np.add.outer(np.arange(70) // 6, np.arange(300) // 9) % 5).astype(np.int32)     # blocks of 6 x 9 cells, five ids, many saddles
    big[rng.random(big.shape) < 0.03] = ND
    big[20:50, 100:200] = 9
    big[30:40, 120:180] = ND
    big[33:36, 140:150] = 9
    g["blocks_70x300"] = big
    g["checker_64x65"] = np.fromfunction(lambda r, c: 1 + (r + c) % 2, (64, 65), dtype=np.int64).astype(np.int32)
    g["stripes_33x64"] = np.fromfunction(lambda r, c: (r + c) % 3, (33, 64), dtype=np.int64).astype(np.int32)
    g["random_68x12"] = rng.integers(0, 2, (68, 12)).astype(np.int32)
    g["single_id_40x64"] = np.full((40, 64), 5, np.int32)    # 2560 cells of one id: the second block has no edge of a row above it
    for k in ("plain:w_plain", "plain:w_outlets", "plain:w_sw", "holes:w_plain", "geographic:w_outlets"):
        g[k] = RECORDED[k]
    return g


GRIDS = _grids()
_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = M.polygonize(GRIDS[name])
    return _MODELS[name]


def tensor_of(w, offset_cells):
    """w on the device, starting offset_cells * 4 bytes past a 16-byte boundary."""
    flat = torch.empty(w.size + 4, dtype=torch.int32, device="cuda:0")
    assert flat.data_ptr() % 16 == 0
    t = flat[offset_cells:offset_cells + w.size].view(w.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(w)))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * offset_cells
    return t


@pytest.mark.parametrize("form", ["numpy", "tensor", "tensor_off_16"])
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_polygonize_equals_the_model(ctx, name, form):
    w, m = GRIDS[name], model(name)
    arg = w if form == "numpy" else tensor_of(w, 0 if form == "tensor" else 1)
    before = None if form == "numpy" else arg.clone()
    with ctx.polygonize(arg, ND) as got:
        assert M.same(got, m) and got.edges == len(m.keys)
        assert set(got.phases) == {"count", "scan", "emit", "download", "rings"} and all(v >= 0 for v in got.phases.values())
    if before is not None:
        assert torch.equal(arg, before)


def test_stats_and_module_level_call(ctx):
    w, m = GRIDS["cut"], model("cut")
    pg, st = ctx.polygonize(w, stats=True)
    with pg:
        assert M.same(pg, m) and "ms_total" in st
    with T.polygonize(w) as pg:
        assert pg.features() == M.features(m)
    other = np.where(w == ND, -9, w).astype(np.int32)       # another nodata value: -5 keeps being an id
    with ctx.polygonize(other, -9) as pg:
        assert M.same(pg, m)


def strip_parts(ctx, w, cuts, check_edges=None):
    """The edge parts of w cut at the rows `cuts`, each strip an array of its own with the neighbours' rows (or poison beyond the raster) as halo rows."""
    from taudem_amd.distributed import StripPipeline

    ny, nx = w.shape
    bounds = [0] + list(cuts) + [ny]
    parts = []
    for y0, y1 in zip(bounds[:-1], bounds[1:]):
        arr = np.full((y1 - y0 + 2, nx), POISON, np.int32)
        lo, hi = max(y0 - 1, 0), min(y1 + 1, ny)
        arr[lo - (y0 - 1):hi - (y0 - 1)] = w[lo:hi]
        t = torch.from_numpy(arr).to("cuda:0")
        part, st = StripPipeline(ctx, None, nx, y1 - y0).polygonize_edges(t, y0, ny, ND)
        assert torch.equal(t.cpu(), torch.from_numpy(arr)), "no row of the strip array is written, halo rows included"
        assert "ms_total" in st
        parts.append(part)
    return parts


def cuts_of(ny, how):
    if how == "rows":
        return list(range(1, ny))
    return sorted({max(1, min(ny - 1, (k * ny) // how)) for k in range(1, how)}) if ny > 1 else []


@pytest.mark.parametrize("how", [2, 3, "rows"])
@pytest.mark.parametrize("name", ["cut", "nested", "saddle", "checker_64x65", "stripes_33x64", "blocks_70x300", "plain:w_plain", "column_41x1", "row_1x37"])
def test_strips_equal_one_device(ctx, name, how):
    w, m = GRIDS[name], model(name)
    ny, nx = w.shape
    cuts = cuts_of(ny, how)
    parts = strip_parts(ctx, w, cuts)
    keys = np.concatenate([api.polygonize_edges(p)[0] for p in parts]) if parts else np.zeros(0, np.int64)
    nxt = np.concatenate([api.polygonize_edges(p)[1] for p in parts])
    ids = np.concatenate([api.polygonize_edges(p)[2] for p in parts])
    assert np.array_equal(keys, m.keys) and np.array_equal(nxt, m.next_keys) and np.array_equal(ids, m.edge_ids), "global keys, in key order over the strips"
    with T.Polygons(parts=parts, nx=nx, ny=ny) as got, ctx.polygonize(w, ND) as one:
        assert M.same(got, one) and M.same(got, m)


def test_cut_rows_carry_regions_saddles_and_holes():
    """What the strip tests claim about the case `cut`: a cut at row 3 (cuts at 2 and 3 of 6 rows, and every row) crosses a region, a hole and a saddle."""
    w = GRIDS["cut"]
    assert w[2, 2] == ND and w[3, 2] == 3 and w[2, 1] == 3                       # the hole of id 3 ends on the cut
    assert w[2, 4] == 1 and w[3, 4] == 2 and w[2, 5] == 1 and w[3, 5] == 1       # ids change across and along the cut
    assert w[3, 4] == w[4, 3] == 2 and w[3, 3] != 2 and w[4, 4] != 2             # a saddle of id 2 at the vertex (4, 4), on the cut after row 3
    assert cuts_of(6, 2) == [3] and cuts_of(6, 3) == [2, 4]


def test_same_bytes_every_run(ctx):
    w = GRIDS["blocks_70x300"]
    t = tensor_of(w, 0)
    from taudem_amd.distributed import StripPipeline

    arr = torch.full((w.shape[0] + 2, w.shape[1]), POISON, dtype=torch.int32, device="cuda:0")
    arr[1:-1] = t
    runs = []
    for _ in range(3):
        part, _ = StripPipeline(ctx, None, w.shape[1], w.shape[0]).polygonize_edges(arr, 0, w.shape[0], ND)
        runs.append([a.tobytes() for a in api.polygonize_edges(part)])
        T.load().tdx_polygonize_edges_free(part)
    assert runs[0] == runs[1] == runs[2]


# ---- the command-line tool
GT = (440000.5, 30.0, 0.0, 4600000.25, 0.0, -30.0)


def _tool(args, gpus=None):
    return subprocess.run([EXE] + (["--gpus", str(gpus)] if gpus else []) + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def _world(ring):
    return [(GT[0] + c * GT[1], GT[3] + r * GT[5]) for c, r in ring]


@pytest.mark.parametrize("name", ["cut", "plain:w_plain"])
def test_tool_writes_the_models_polygons(name, tmp_path):
    w, feats = GRIDS[name], M.features(model(name))
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("w.tif"), w, ND, geotransform=GT)
    r = _tool(["-w", f("w.tif"), "-poly", f("ws.shp")])
    assert r.returncode == 0, r.stdout + r.stderr
    nring = sum(len(p) for _, _, polys in feats for p in polys)
    nvert = sum(len(ring) for _, _, polys in feats for p in polys for ring in p)
    assert f"Polygons: {len(feats)} features, {sum(len(polys) for _, _, polys in feats)} polygons, {nring} rings, {nvert} vertices\n" in r.stdout
    assert r.stdout.startswith("WatershedGridToShapefile version ") and "Processes: 1\n" in r.stdout and "Total time: " in r.stdout
    got = P.shapefile_features(f("ws.shp"))
    assert [(int(a["gridcode"]), int(a["cells"])) for a, _ in got] == [(a, cells) for a, cells, _ in feats]
    assert [rings for _, rings in got] == [[_world(ring) for p in polys for ring in p] for _, _, polys in feats]
    r = _tool(["-w", f("w.tif"), "-poly", f("ws.geojson")])
    assert r.returncode == 0, r.stdout + r.stderr
    gj, _ = P.geojson(f("ws.geojson"))
    assert [(a, polys) for a, polys in gj] == [({"gridcode": a, "cells": cells}, [[_world(ring)[::-1] for ring in p] for p in polys]) for a, cells, polys in feats]
    # three strips: the same bytes
    for out in ("ws3.shp", "ws3.geojson"):
        r = _tool(["-w", f("w.tif"), "-poly", f(out)], gpus=3)
        assert r.returncode == 0 and "Processes: 3\n" in r.stdout, r.stdout + r.stderr
    for a, b in (("ws.shp", "ws3.shp"), ("ws.shx", "ws3.shx"), ("ws.dbf", "ws3.dbf"), ("ws.geojson", "ws3.geojson")):
        assert open(f(a), "rb").read() == open(f(b), "rb").read(), (a, b)


def test_tool_refuses_an_unsupported_extension(tmp_path):
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("w.tif"), GRIDS["cut"], ND, geotransform=GT)
    before = sorted(os.listdir(tmp_path))
    r = _tool(["-w", f("w.tif"), "-poly", f("ws.gpkg")])
    assert r.returncode == 2 and "watershedgridtoshp cannot write" in r.stderr and "version" not in r.stdout   # refused before anything is read
    r = _tool(["-w", f("missing.tif"), "-poly", f("ws.shp")])
    assert r.returncode == 21 and r.stdout.endswith(f"Error opening file {f('missing.tif')}.\n")
    assert _tool(["-w", f("w.tif")]).stdout.startswith("Usage: ")
    assert sorted(os.listdir(tmp_path)) == before


def test_tool_writes_an_empty_layer(tmp_path):
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("w.tif"), GRIDS["all_nodata"], ND, geotransform=GT)
    r = _tool(["-w", f("w.tif"), "-poly", f("none.shp")])
    assert r.returncode == 0 and "Polygons: 0 features, 0 polygons, 0 rings, 0 vertices\n" in r.stdout, r.stdout + r.stderr
    assert P.shp(f("none.shp"))["records"] == []
