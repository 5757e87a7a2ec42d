"""The ring builder of the watershed polygons (tdx_polygonize_edges_create -> tdx_polygonize_rings, taudem_amd.Polygons(parts=...)) on a machine
without a GPU: the edges come from the model (tests/polygonize_model.py), go in as one part and as 2, 3 and per-row parts, and the result equals the
model's polygons exactly - ids, cells, the three offset lists and the vertices.  Parts out of order, a missing part and a successor that no edge
carries are refused with TDX_ERR_ARG and a reason.  The header include/taudem_amd_polygonize.h is held the way the other extension headers are."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import polygonize_model as M
import taudem_amd as T
from taudem_amd import _lib, api, tools
from test_polygonize_model import HAND, RECORDED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "taudem_amd", "bin", "watershedgridtoshp")
GRIDS = dict(HAND, **{k: RECORDED[k] for k in sorted(RECORDED) if k.split(":")[0] in ("plain", "holes", "small")})
_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = M.polygonize(GRIDS[name])
    return _MODELS[name]


def parts_of(m, nx, cuts):
    """The model's edges cut into parts at the rows `cuts` (ascending, inside the raster)."""
    bounds = [0] + [int(np.searchsorted(m.keys, r * nx * 4)) for r in cuts] + [len(m.keys)]
    return [api.polygonize_edges_create(m.keys[a:b], m.next_keys[a:b], m.edge_ids[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]


def cuts_of(ny, how):
    if how == "rows":
        return list(range(1, ny))
    return sorted({max(1, min(ny - 1, (k * ny) // how)) for k in range(1, how)}) if ny > 1 else []


@pytest.mark.parametrize("how", [1, 2, 3, "rows"])
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_rings_equal_the_model(name, how):
    w, m = GRIDS[name], model(name)
    ny, nx = w.shape
    with T.Polygons(parts=parts_of(m, nx, cuts_of(ny, how)), nx=nx, ny=ny) as got:
        assert M.same(got, m)
        assert got.edges == len(m.keys) and got.features() == M.features(m)


def test_edges_round_trip():
    m = model("cut")
    part = api.polygonize_edges_create(m.keys, m.next_keys, m.edge_ids)
    try:
        k, n, i = api.polygonize_edges(part)
        assert np.array_equal(k, m.keys) and np.array_equal(n, m.next_keys) and np.array_equal(i, m.edge_ids)
    finally:
        T.load().tdx_polygonize_edges_free(part)


def _refused(parts, nx, ny, reason):
    try:
        with pytest.raises(T.TdxError, match=reason) as e:
            T.Polygons(parts=parts, nx=nx, ny=ny)
        assert e.value.code == _lib.TDX_ERR_ARG
    finally:
        for p in parts:
            T.load().tdx_polygonize_edges_free(p)


def test_malformed_edges_are_refused_not_walked():
    w, m = GRIDS["cut"], model("cut")
    ny, nx = w.shape
    a, b, c = parts_of(m, nx, [2, 4])
    _refused([b, a, c], nx, ny, "do not ascend")                       # parts out of order
    a, b, c = parts_of(m, nx, [2, 4])
    T.load().tdx_polygonize_edges_free(b)
    _refused([a, c], nx, ny, "not among the edges")                     # a strip missing
    nxt = m.next_keys.copy()
    nxt[3] = int(m.keys[-1]) + 1 if (int(m.keys[-1]) + 1) not in set(m.keys.tolist()) else int(m.keys[-1]) + 2
    _refused([api.polygonize_edges_create(m.keys, nxt, m.edge_ids)], nx, ny, "not among the edges|does not start")
    nxt = m.next_keys.copy()
    nxt[0] = nxt[1]                                                      # two edges with one successor
    _refused([api.polygonize_edges_create(m.keys, nxt, m.edge_ids)], nx, ny, "does not start|permutation")
    _refused([api.polygonize_edges_create(m.keys + 4 * nx * ny, m.next_keys, m.edge_ids)], nx, ny, "outside the raster")
    ids = m.edge_ids.copy()
    ids[0] += 1
    _refused([api.polygonize_edges_create(m.keys, m.next_keys, ids)], nx, ny, "id changes")
    with pytest.raises(ValueError):
        api.polygonize_edges_create([0, 1], [1], [1, 1])


def test_empty_parts_give_an_empty_layer(tmp_path):
    with T.Polygons(parts=[api.polygonize_edges_create([], [], [])], nx=4, ny=3) as got:
        assert got.ids.size == 0 and got.poly_first.tolist() == [0] and got.ring_first.tolist() == [0] and got.vert_first.tolist() == [0]
        got.write(str(tmp_path / "empty.geojson"))
    assert '"features": [\n]' in open(tmp_path / "empty.geojson").read()


def test_header_library_signatures_and_names():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taudem_amd_polygonize.h")).read(), flags=re.S)
    decl = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(tdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}
    lib = T.load()
    assert '#include "taudem_amd_polygonize.h"' in open(os.path.join(ROOT, "include", "taudem_amd.h")).read()
    assert set(decl) == set(_lib.POLYGONIZE_SYMBOLS) and decl["tdx_polygonize_edges_strip"] == 10 and decl["tdx_tool_watershedgridtoshp"] == 2
    for other in (_lib.EXPORTED_SYMBOLS, _lib.STREAMNET_SYMBOLS, _lib.OUTLETS_SYMBOLS, _lib.INDICES_SYMBOLS, _lib.EDITRASTER_SYMBOLS, _lib.CATCHOUTLETS_SYMBOLS):
        assert not set(decl) & set(other)
    for sym, nparams in decl.items():
        assert len(getattr(lib, sym).argtypes) == nparams, sym
    for sym in ("tdx_polygonize", "tdx_polygonize_dev", "tdx_polygonize_edges_strip", "tdx_polygonize_edges_create", "tdx_polygonize_rings", "tdx_polygons_write",
                "tdx_tool_watershedgridtoshp"):
        fn = getattr(lib, sym)
        args = [t() for t in fn.argtypes]
        if sym == "tdx_polygonize_edges_create":
            args[3] = C.c_int64(1)   # one edge without columns
        assert fn(*args) == _lib.TDX_ERR_ARG and _lib.last_error(None) == sym + ": bad argument", sym
    assert lib.tdx_polygons_count(None, None, None, None, None) == 0 and lib.tdx_polygonize_edges_count(None) == 0
    lib.tdx_polygons_free(None)
    lib.tdx_polygonize_edges_free(None)
    assert _lib.POLYGONIZE_PHASES == ("count", "scan", "emit", "download", "rings")
    h = open(os.path.join(ROOT, "include", "taudem_amd_polygonize.h")).read()
    for k, name in enumerate(_lib.POLYGONIZE_PHASES):
        assert re.search(rf"#define TDX_POLYGONIZE_{name.upper()} {k}\b", h)
    assert f"#define TDX_POLYGONIZE_PHASES {len(_lib.POLYGONIZE_PHASES)}" in h


def test_python_surface_and_makefile():
    from taudem_amd.distributed import StripPipeline

    par = inspect.signature(T.Context.polygonize).parameters
    assert list(par) == ["self", "w", "nodata", "stats"] and par["nodata"].default == -2147483647 and par["stats"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "polygonize" not in vars(T.Context) and "polygonize_edges" not in vars(StripPipeline)   # mixins: the pinned method sets stay
    assert list(inspect.signature(StripPipeline.polygonize_edges).parameters) == ["self", "w", "row0", "ny_total", "nodata"]
    assert list(inspect.signature(tools.watershedgridtoshp).parameters) == ["wfile", "polyfile"] and callable(T.polygonize)
    assert callable(T.Polygons.write) and callable(T.Polygons.__enter__) and callable(T.Polygons.close)
    mk = open(os.path.join(ROOT, "taudem_amd", "csrc", "Makefile")).read()
    assert " watershedgridtoshp" in next(ln for ln in mk.splitlines() if ln.startswith("TOOLS")) and os.access(EXE, os.X_OK)
    assert " polygonize.hip" in next(ln for ln in mk.splitlines() if ln.startswith("HIPSRC"))
    assert " polygon_rings.cpp" in next(ln for ln in mk.splitlines() if ln.startswith("CPPSRC"))
