"""The device ring builder (Context.polygonize_rings(rings="device"), Polygons(parts=, ctx=, rings="device"), watershedgridtoshp -rings device)
against the model (tests/polygonize_model.py) and against the host ring builder, which is the default and the witness: ids, cells, the three offset
lists and the vertices are equal exactly - the output is integers, there is no tolerance.

Shapes: every grid of tests/test_gpu_polygonize.py in the three array forms (1 x 1, 1 x 37, 41 x 1, the checkerboard of 4 160 four-edge rings, the
stripes whose inner vertices are all saddles, 70 x 300 across block boundaries, nested hole and island, all nodata with no edge at all, negative ids and
0, the recorded StreamNet grids); one ring of 2 N + 2 edges for N on both sides of a jump round (31, 32, 33, 1023, 1024); a serpentine ring of about
9.7 k edges beside 500 four-edge rings; holes stacked three and five deep in one column (the owner chain hole -> hole -> outer ring), two holes side
by side whose walks end on different rings, a hole 298 rows below the outer ring's top (five strides of the walking wave), a hole that holds an island
that holds a hole (tests/polygon_rings_cases.py); fifty seeded random grids."""
import math
import os

import numpy as np
import pytest

import polygonize_model as M
import taudem_amd as T
from polygon_rings_cases import CASES, random_grid
from taudem_amd import _lib, api
from test_gpu_polygonize import GRIDS as BASE
from test_gpu_polygonize import GT, ND, _tool, cuts_of, strip_parts, tensor_of

pytestmark = pytest.mark.gpu

LENGTHS = {f"row_of_{n}": np.full((1, n), 4, np.int32) for n in (31, 32, 33, 1023, 1024)}
GRIDS = dict(BASE, **CASES, **LENGTHS)
ARRAYS = ("ids", "cells", "poly_first", "ring_first", "vert_first", "vertices")
_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = M.polygonize(GRIDS[name])
    return _MODELS[name]


def same_bytes(a, b):
    for k in ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    return True


def round_bound(edges):
    return (math.ceil(math.log2(edges)) if edges > 1 else 0) + 1


@pytest.mark.parametrize("form", ["numpy", "tensor", "tensor_off_16"])
@pytest.mark.parametrize("name", sorted(BASE))
def test_device_rings_equal_the_model_and_the_host(ctx, name, form):
    w, m = GRIDS[name], model(name)
    arg = w if form == "numpy" else tensor_of(w, 0 if form == "tensor" else 1)
    with ctx.polygonize_rings(arg, ND, rings="device") as got, ctx.polygonize_rings(arg, ND, rings="host") as host:
        assert M.same(got, m) and same_bytes(got, host)
        assert got.edges == host.edges == len(m.keys)
        assert host.ring_phases == {} and (got.edges == 0 or got.ring_rounds <= round_bound(got.edges))


@pytest.mark.parametrize("name", sorted(dict(CASES, **LENGTHS)))
def test_ring_lengths_and_holes(ctx, name):
    w, m = GRIDS[name], model(name)
    with ctx.polygonize_rings(w, ND, rings="device") as got, ctx.polygonize(w, ND) as host:
        assert M.same(got, m) and same_bytes(got, host) and got.edges == len(m.keys)
        assert 1 <= got.ring_rounds <= round_bound(got.edges)


def parts_of(m, nx, cuts):
    bounds = [0] + [int(np.searchsorted(m.keys, r * nx * 4)) for r in cuts] + [len(m.keys)]
    return [api.polygonize_edges_create(m.keys[a:b], m.next_keys[a:b], m.edge_ids[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]


def _refused(ctx, parts, nx, ny, reason):
    try:
        with pytest.raises(T.TdxError, match=reason) as e:
            T.Polygons(parts=parts, nx=nx, ny=ny, ctx=ctx, rings="device")
        assert e.value.code == _lib.TDX_ERR_ARG and _lib.last_error(None)
    finally:
        for p in parts:
            T.load().tdx_polygonize_edges_free(p)


def test_malformed_edges_are_refused_on_the_device(ctx):
    """Each class of malformed edges that tests/test_polygonize_host.py builds for the host builder, with the host's reasons."""
    w, m = GRIDS["cut"], model("cut")
    ny, nx = w.shape
    a, b, c = parts_of(m, nx, [2, 4])
    _refused(ctx, [b, a, c], nx, ny, "do not ascend")
    a, b, c = parts_of(m, nx, [2, 4])
    T.load().tdx_polygonize_edges_free(b)
    _refused(ctx, [a, c], nx, ny, "not among the edges")
    nxt = m.next_keys.copy()
    nxt[3] = int(m.keys[-1]) + 1 if (int(m.keys[-1]) + 1) not in set(m.keys.tolist()) else int(m.keys[-1]) + 2
    _refused(ctx, [api.polygonize_edges_create(m.keys, nxt, m.edge_ids)], nx, ny, "not among the edges|does not start")
    nxt = m.next_keys.copy()
    nxt[0] = nxt[1]
    _refused(ctx, [api.polygonize_edges_create(m.keys, nxt, m.edge_ids)], nx, ny, "does not start|permutation")
    _refused(ctx, [api.polygonize_edges_create(m.keys + 4 * nx * ny, m.next_keys, m.edge_ids)], nx, ny, "outside the raster")
    ids = m.edge_ids.copy()
    ids[0] += 1
    _refused(ctx, [api.polygonize_edges_create(m.keys, m.next_keys, ids)], nx, ny, "id changes")
    with T.Polygons(parts=parts_of(m, nx, []), nx=nx, ny=ny, ctx=ctx, rings="device") as got:   # the context works on after the refusals
        assert M.same(got, m)


def test_hand_made_parts_equal_the_model(ctx):
    for name in ("cut", "nested", "hole_island_hole", "holes_stacked_5"):
        w, m = GRIDS[name], model(name)
        ny, nx = w.shape
        for how in (1, 2, 3, "rows"):
            with T.Polygons(parts=parts_of(m, nx, cuts_of(ny, how)), nx=nx, ny=ny, ctx=ctx, rings="device") as got:
                assert M.same(got, m) and got.edges == len(m.keys) and set(got.ring_phases) == set(_lib.POLYGONIZE_RING_PHASES)
    with T.Polygons(parts=[api.polygonize_edges_create([], [], [])], nx=4, ny=3, ctx=ctx, rings="device") as got:
        assert got.ids.size == 0 and got.poly_first.tolist() == [0] and got.ring_first.tolist() == [0] and got.vert_first.tolist() == [0]


@pytest.mark.parametrize("how", [2, 3, "rows"])
@pytest.mark.parametrize("name", ["cut", "nested", "checker_64x65", "blocks_70x300", "plain:w_plain"])
def test_strip_parts_closed_on_the_device_equal_one_device(ctx, name, how):
    w, m = GRIDS[name], model(name)
    ny, nx = w.shape
    parts = strip_parts(ctx, w, cuts_of(ny, how))
    with T.Polygons(parts=parts, nx=nx, ny=ny, ctx=ctx, rings="device") as got, ctx.polygonize_rings(w, ND, rings="device") as one:
        assert same_bytes(got, one) and M.same(got, m)


@pytest.mark.parametrize("block", range(5))
def test_random_grids(ctx, block):
    for seed in range(10 * block, 10 * block + 10):
        w = random_grid(seed)
        m = M.polygonize(w)
        with ctx.polygonize_rings(w, ND, rings="device") as got, ctx.polygonize(w, ND) as host:
            assert M.same(got, m) and same_bytes(got, host), seed


def test_same_bytes_every_run(ctx):
    t = tensor_of(GRIDS["blocks_70x300"], 0)
    runs = []
    for _ in range(2):
        with ctx.polygonize_rings(t, ND, rings="device") as got:
            runs.append([getattr(got, k).tobytes() for k in ARRAYS] + [got.ring_rounds])
    assert runs[0] == runs[1]


def test_phases_and_ring_phases(ctx):
    w = GRIDS["blocks_70x300"]
    with ctx.polygonize_rings(w, ND, rings="device") as got, ctx.polygonize(w, ND) as host, T.polygonize(w, ND, rings="device") as mod:
        assert tuple(got.phases) == tuple(host.phases) == ("count", "scan", "emit", "download", "rings") and all(v >= 0 for v in got.phases.values())
        assert tuple(got.ring_phases) == ("successor", "validate", "label", "per_ring", "rank", "holes", "order", "scatter")
        assert all(v >= 0 for v in got.ring_phases.values()) and abs(sum(got.ring_phases.values()) - got.phases["rings"]) < 1e-6
        assert 1 <= got.ring_rounds <= round_bound(got.edges) and got.ring_workspace_bytes >= 33 * got.edges
        assert host.ring_phases == {} and host.ring_rounds == 0 and host.ring_workspace_bytes == 0
        assert same_bytes(mod, host)
    pg, st = ctx.polygonize_rings(w, ND, rings="device", stats=True)
    with pg:
        assert "ms_total" in st
    with pytest.raises(ValueError):
        ctx.polygonize_rings(w, ND, rings="elsewhere")


@pytest.mark.parametrize("name", ["cut", "plain:w_plain"])
def test_tool_with_device_rings_writes_the_host_paths_bytes(name, tmp_path):
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("w.tif"), GRIDS[name], ND, geotransform=GT)
    for out in ("host.shp", "host.geojson"):
        r = _tool(["-w", f("w.tif"), "-poly", f(out), "-rings", "host"])
        assert r.returncode == 0, r.stdout + r.stderr
    for tag, gpus in (("dev", None), ("dev2", 2)):
        for ext in ("shp", "geojson"):
            r = _tool(["-w", f("w.tif"), "-poly", f(f"{tag}.{ext}"), "-rings", "device"], gpus=gpus)
            assert r.returncode == 0 and f"Processes: {gpus or 1}\n" in r.stdout, r.stdout + r.stderr
        for ext in ("shp", "shx", "dbf", "geojson"):
            assert open(f(f"{tag}.{ext}"), "rb").read() == open(f(f"host.{ext}"), "rb").read(), (tag, ext)
    before = sorted(os.listdir(tmp_path))
    r = _tool(["-w", f("w.tif"), "-poly", f("no.shp"), "-rings", "nonsense"])
    assert r.returncode == 2 and "host or device" in r.stderr and "version" not in r.stdout and sorted(os.listdir(tmp_path)) == before
