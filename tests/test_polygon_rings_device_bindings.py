"""The surface of the device ring builder without a GPU: the new symbols are declared in include/taudem_amd_polygonize.h, exported by the library and
bound with the header's parameter counts; they refuse null arguments; the choice of the ring builder is a word, "host" or "device", everywhere, and
any other word is refused before a device is touched; the host path reports no ring sub-phases; the command-line tool refuses another word with exit
status 2 before anything is read."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import polygonize_model as M
import taudem_amd as T
from taudem_amd import _lib, api, tools
from test_polygonize_model import HAND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "taudem_amd", "bin", "watershedgridtoshp")
NEW = {"tdx_polygonize_gpu_rings": 7, "tdx_polygonize_gpu_rings_dev": 7, "tdx_polygonize_rings_gpu": 7, "tdx_polygons_ring_phases": 4, "tdx_tool_set_polygon_rings": 1}


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taudem_amd_polygonize.h")).read(), flags=re.S)
    decl = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(tdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}
    lib = T.load()
    for sym, nparams in NEW.items():
        assert decl.get(sym) == nparams and sym in _lib.POLYGONIZE_SYMBOLS and len(getattr(lib, sym).argtypes) == nparams, sym
    for sym in ("tdx_polygonize_gpu_rings", "tdx_polygonize_gpu_rings_dev", "tdx_polygonize_rings_gpu"):
        fn = getattr(lib, sym)
        assert fn(*[t() for t in fn.argtypes]) == _lib.TDX_ERR_ARG and _lib.last_error(None) == sym + ": bad argument", sym
    ms, rounds, wsb = np.full(len(_lib.POLYGONIZE_RING_PHASES), 7.0), C.c_int64(5), C.c_int64(5)
    assert lib.tdx_polygons_ring_phases(None, ms.ctypes.data_as(C.c_void_p), C.byref(rounds), C.byref(wsb)) == 0
    assert not ms.any() and rounds.value == 0 and wsb.value == 0
    h = open(os.path.join(ROOT, "include", "taudem_amd_polygonize.h")).read()
    for k, name in enumerate(_lib.POLYGONIZE_RING_PHASES):
        assert re.search(rf"#define TDX_POLYGONIZE_RING_{name.upper()} {k}\b", h)
    assert f"#define TDX_POLYGONIZE_RING_PHASES {len(_lib.POLYGONIZE_RING_PHASES)}" in h and "#define TDX_POLYGONIZE_PHASES 5" in h
    mk = open(os.path.join(ROOT, "taudem_amd", "csrc", "Makefile")).read()
    assert " polygon_rings_device.hip" in next(ln for ln in mk.splitlines() if ln.startswith("HIPSRC"))


def test_the_tool_setting_takes_host_or_device():
    lib = T.load()
    assert lib.tdx_tool_set_polygon_rings(2) == _lib.TDX_ERR_ARG and lib.tdx_tool_set_polygon_rings(-1) == _lib.TDX_ERR_ARG
    assert lib.tdx_tool_set_polygon_rings(1) == 0 and lib.tdx_tool_set_polygon_rings(0) == 0
    assert tools.set_polygon_rings("device") == 0 and tools.set_polygon_rings("host") == 0 and tools.set_polygon_rings() == 0
    with pytest.raises(ValueError):
        tools.set_polygon_rings("elsewhere")
    assert list(inspect.signature(tools.watershedgridtoshp).parameters) == ["wfile", "polyfile"]


def test_rings_is_a_word_everywhere():
    par = inspect.signature(T.Context.polygonize_rings).parameters
    assert list(par) == ["self", "w", "nodata", "rings", "stats"] and par["rings"].default == "host" and par["rings"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "polygonize_rings" not in vars(T.Context)   # a mixin's, like polygonize
    assert inspect.signature(T.polygonize).parameters["rings"].default == "host"
    par = inspect.signature(T.Polygons.__init__).parameters
    assert list(par) == ["self", "handle", "parts", "nx", "ny", "ctx", "rings"] and par["ctx"].default is None and par["rings"].default == "host"
    w = HAND["cut"]
    with pytest.raises(ValueError, match="elsewhere"):
        T.polygonize(w, rings="elsewhere")            # before a context is made
    m = M.polygonize(w)
    part = api.polygonize_edges_create(m.keys, m.next_keys, m.edge_ids)
    try:
        with pytest.raises(ValueError, match="elsewhere"):
            T.Polygons(parts=[part], nx=w.shape[1], ny=w.shape[0], rings="elsewhere")
        with pytest.raises(ValueError, match="ctx"):
            T.Polygons(parts=[part], nx=w.shape[1], ny=w.shape[0], rings="device")
    finally:
        T.load().tdx_polygonize_edges_free(part)


def test_the_host_path_reports_no_ring_phases():
    w = HAND["nested"]
    m = M.polygonize(w)
    with T.Polygons(parts=[api.polygonize_edges_create(m.keys, m.next_keys, m.edge_ids)], nx=w.shape[1], ny=w.shape[0]) as got:
        assert M.same(got, m) and got.ring_phases == {} and got.ring_rounds == 0 and got.ring_workspace_bytes == 0
        assert tuple(got.phases) == ("count", "scan", "emit", "download", "rings")


def test_tool_refuses_another_word_before_anything_is_read(tmp_path):
    before = sorted(os.listdir(tmp_path))
    r = subprocess.run([EXE, "-w", str(tmp_path / "missing.tif"), "-poly", str(tmp_path / "ws.shp"), "-rings", "nonsense"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "host or device" in r.stderr and r.stdout == "" and sorted(os.listdir(tmp_path)) == before
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.stdout.startswith("Usage: ") and "[-rings host|device]" in r.stdout
