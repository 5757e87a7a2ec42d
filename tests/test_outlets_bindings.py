"""The outlet tools' part of the C ABI (include/taudem_amd_outlets.h, which include/taudem_amd.h includes) held the way
tests/test_streamnet_bindings.py holds StreamNet's: the library exports every symbol the header declares, taudem_amd/_lib.py has a ctypes signature
with as many arguments as the declaration for each and binds no other, and the compute forms reject a null context with TDX_ERR_ARG and their own
"<symbol>: bad argument" text before they touch HIP.  The order in which Context's and StripPipeline's methods hand their arguments to the library
is read off a recording stand-in for it, with the stand-in tensors of tests/binding_recorder.py.  No GPU is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import binding_recorder as B
import taudem_amd as T
from taudem_amd import _lib, tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPUTE = ("tdx_moveoutlets", "tdx_moveoutlets_dev", "tdx_moveoutlets_strip", "tdx_connectdown", "tdx_connectdown_dev", "tdx_connectdown_strip",
           "tdx_connectdown_walk_strip", "tdx_connectdown_merge", "tdx_connectdown_points_set_moved", "tdx_points_write", "tdx_tool_moveoutletstostrm",
           "tdx_tool_connectdown")


def _declarations():
    """symbol -> number of parameters, of the extension header"""
    text = open(os.path.join(ROOT, "include", "taudem_amd_outlets.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(tdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_main_header_includes_the_extension():
    text = open(os.path.join(ROOT, "include", "taudem_amd.h")).read()
    assert '#include "taudem_amd_outlets.h"' in text


def test_library_exports_every_declared_symbol_with_a_signature():
    lib, decl = T.load(), _declarations()
    assert set(decl) == set(_lib.OUTLETS_SYMBOLS) and set(COMPUTE) <= set(decl)
    assert not set(decl) & set(_lib.EXPORTED_SYMBOLS)
    for sym, nparams in decl.items():
        fn = getattr(lib, sym)
        assert fn.restype is _lib._OUTLETS_SIGNATURES[sym][0] and len(fn.argtypes) == nparams, sym
    text = open(os.path.join(ROOT, "include", "taudem_amd_outlets.h")).read()
    assert f"#define TDX_CONNECTDOWN_MAX_ID {_lib.CONNECTDOWN_MAX_ID} " in text and _lib.CONNECTDOWN_MAX_ID == 2**27 - 1
    assert len(_lib.CONNECTDOWN_PHASES) == int(re.search(r"#define TDX_CONNECTDOWN_PHASES (\d+)", text).group(1))


@pytest.mark.parametrize("sym", COMPUTE)
def test_null_arguments_are_a_bad_argument(sym):
    fn = getattr(T.load(), sym)
    rc = fn(*[t() for t in fn.argtypes])   # null context, null pointers, zeros
    assert rc == _lib.TDX_ERR_ARG
    assert _lib.last_error(None) == sym + ": bad argument"


def test_points_accessors_take_a_null_handle():
    lib = T.load()
    assert lib.tdx_connectdown_points_count(None) == 0
    lib.tdx_connectdown_points_copy(None, None, None, None, None, None, None, None, None)
    lib.tdx_connectdown_points_free(None)


def test_merge_takes_the_first_strip_unless_a_later_one_is_greater():
    """host code: two empty parts merge to no points (parts with points come from a device: tests/test_gpu_outlets_strips.py)"""
    lib = T.load()
    out = C.c_void_p()
    arr = (C.c_void_p * 2)(None, None)
    assert lib.tdx_connectdown_merge(C.cast(arr, C.c_void_p), 2, C.byref(out)) == _lib.TDX_ERR_ARG and not out.value


def test_unsupported_outputs_are_refused_before_anything_is_read(tmp_path, capfd):
    missing = str(tmp_path / "missing.tif")
    rc = tools.outletstosrc(missing, missing, missing, outletmoveddatasrc=str(tmp_path / "moved.kml"))
    out = capfd.readouterr()
    assert rc == _lib.TDX_ERR_ARG and ".geojson" in out.err and "version" not in out.out and not os.listdir(tmp_path)
    rc = tools.connectdown(missing, missing, missing, str(tmp_path / "o.shp"), movedoutletdatasrc=str(tmp_path / "od.gpkg"))
    out = capfd.readouterr()
    assert rc == _lib.TDX_ERR_ARG and "od.gpkg" in out.err and "version" not in out.out and not os.listdir(tmp_path)
    assert tools.moveoutletstostrm is tools.outletstosrc


def test_stage_methods_exist():
    from taudem_amd.distributed import StripPipeline

    assert callable(T.Context.moveoutletstostrm) and callable(T.Context.connectdown) and callable(T.moveoutletstostrm) and callable(T.connectdown)
    assert callable(T.write_points) and callable(T.ConnectDownPoints)
    assert callable(StripPipeline.moveoutletstostrm) and callable(StripPipeline.connectdown_argmax) and callable(StripPipeline.connectdown_walk)
    assert "moveoutletstostrm" not in vars(T.Context) and "connectdown" not in vars(T.Context)      # a mixin's, as tests/test_binding_calls.py counts Context's own


# ---- the order of the arguments that reach the library ------------------------------------------------------------------------------------
class Recording:
    """Stands in for the loaded library: every outlet symbol returns 0 and records its arguments as plain values."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        if symbol not in _lib.OUTLETS_SYMBOLS:
            raise AttributeError(symbol)

        def fn(*args):
            self.calls.append((symbol, args))
            return 0
        return fn


def _plain(v):
    return getattr(v, "value", v)


def _subject(kind):
    rec = Recording()
    ctx = T.Context.__new__(T.Context)
    ctx._lib, ctx._h, ctx.device = rec, C.c_void_p(B.CTX_HANDLE), B.DEVICE
    if kind != "strip":
        return ctx, rec
    from taudem_amd.distributed import StripPipeline

    pipe = StripPipeline.__new__(StripPipeline)
    pipe.ctx, pipe.comm, pipe.nx, pipe.ny_local, pipe.shape, pipe._cp, pipe.torch = ctx, None, B.NX, B.NY_LOCAL, (B.NY_LOCAL + 2, B.NX), C.c_void_p(B.COMM_HANDLE), torch
    return pipe, rec


def _raster(kind, dtype):
    if kind == "host":
        return np.zeros((B.NY, B.NX), dtype)
    shape = (B.NY_LOCAL + 2, B.NX) if kind == "strip" else (B.NY, B.NX)
    return B.FakeTensor(shape, B.TORCH_DT[dtype])


def _ptr(a):
    return B._address(a)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_context_calls_reach_the_library_in_the_headers_order(kind):
    with B.no_device():
        ctx, rec = _subject(kind)
        p, src, w, ad8 = _raster(kind, np.int16), _raster(kind, np.int32), _raster(kind, np.int32), _raster(kind, np.float32)
        rx, ry, rd, st = ctx.moveoutletstostrm(p, src, ([1, 2, 3], [4, 0, 2]), 17, nodata=-5, src_nodata=-6, stats=True)
        res = ctx.connectdown(p, w, ad8, 9, nodata=-5, w_nodata=-7, stats=True)
    suffix = "_dev" if kind == "device" else ""
    (s1, a1), (s2, a2) = rec.calls[0], rec.calls[1]
    assert s1 == "tdx_moveoutlets" + suffix and len(a1) == len(_lib._OUTLETS_SIGNATURES[s1][1])
    a = [_plain(v) for v in a1]
    assert a[0] == B.CTX_HANDLE and a[1:3] == [_ptr(p), _ptr(src)] and a[3:8] == [B.NX, B.NY, -5, -6, 17] and a[10] == 3
    assert a[11:14] == [rx.ctypes.data, ry.ctypes.data, rd.ctypes.data] and rx.dtype == np.int32 and "ms_total" in st
    assert s2 == "tdx_connectdown" + suffix and len(a2) == len(_lib._OUTLETS_SIGNATURES[s2][1])
    a = [_plain(v) for v in a2[:9]]
    assert a[0] == B.CTX_HANDLE and a[1:4] == [_ptr(p), _ptr(w), _ptr(ad8)] and a[4:9] == [B.NX, B.NY, -5, -7, 9]
    assert [c[0] for c in rec.calls[2:]] == ["tdx_connectdown_points_count", "tdx_connectdown_points_copy", "tdx_connectdown_points_free"]
    assert len(res) == 8 and all(isinstance(v, np.ndarray) for v in res[:7]) and res[3].dtype == np.float32


def test_strip_calls_reach_the_library_in_the_headers_order():
    with B.no_device():
        pipe, rec = _subject("strip")
        p, src, w, ad8 = _raster("strip", np.int16), _raster("strip", np.int32), _raster("strip", np.int32), _raster("strip", np.float32)
        state = tuple(np.zeros(4, np.int32) for _ in range(5))
        pipe.moveoutletstostrm(p, src, 30, 100, state[:4], 17, nodata=-5, src_nodata=-6)
        pipe.connectdown_argmax(w, ad8, 30, w_nodata=-7)
        pipe.connectdown_walk(p, w, 30, 100, state, 9)
    (s1, a1), (s2, a2), (s3, a3) = rec.calls
    a = [_plain(v) for v in a1]
    assert s1 == "tdx_moveoutlets_strip" and len(a1) == len(_lib._OUTLETS_SIGNATURES[s1][1])
    assert a[:2] == [B.CTX_HANDLE, B.COMM_HANDLE] and a[2:4] == [_ptr(p), _ptr(src)] and a[4:11] == [B.NX, B.NY_LOCAL, 30, 100, -5, -6, 17]
    assert a[11:15] == [s.ctypes.data for s in state[:4]] and a[15] == 4
    a = [_plain(v) for v in a2]
    assert s2 == "tdx_connectdown_strip" and len(a2) == len(_lib._OUTLETS_SIGNATURES[s2][1])
    assert a[:2] == [B.CTX_HANDLE, B.COMM_HANDLE] and a[2:4] == [_ptr(w), _ptr(ad8)] and a[4:8] == [B.NX, B.NY_LOCAL, 30, -7]
    a = [_plain(v) for v in a3]
    assert s3 == "tdx_connectdown_walk_strip" and len(a3) == len(_lib._OUTLETS_SIGNATURES[s3][1])
    assert a[:2] == [B.CTX_HANDLE, B.COMM_HANDLE] and a[2:4] == [_ptr(p), _ptr(w)] and a[4:9] == [B.NX, B.NY_LOCAL, 30, 100, 9]
    assert a[9:14] == [s.ctypes.data for s in state] and a[14] == 4


def test_bad_state_and_outlets_are_rejected_before_any_call():
    with B.no_device():
        pipe, rec = _subject("strip")
        p, src = _raster("strip", np.int16), _raster("strip", np.int32)
        with pytest.raises(ValueError):
            pipe.moveoutletstostrm(p, src, 0, 10, (np.zeros(3, np.int32), np.zeros(3, np.int64), np.zeros(3, np.int32), np.zeros(3, np.int32)))
        ctx, rec2 = _subject("host")
        with pytest.raises(ValueError):
            ctx.moveoutletstostrm(_raster("host", np.int16), _raster("host", np.int32), ([1, 2], [1]))
    assert not rec.calls and not rec2.calls
