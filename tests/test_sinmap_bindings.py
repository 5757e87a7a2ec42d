"""The SinmapSI part of the C ABI (include/taudem_amd_sinmap.h, which include/taudem_amd.h includes) held the way tests/test_peuker_bindings.py holds the
PeukerDouglas header: the library exports every symbol it declares, taudem_amd/_lib.py has a ctypes signature with as many arguments as the declaration
for each and binds no other, none of them is in another table, and the three compute forms reject a null context with TDX_ERR_ARG and their own
"<symbol>: bad argument" text before they touch HIP.  Context and StripPipeline have the stage method; the shim forwards sindexcombined.  No GPU is needed."""
import inspect
import os
import re

import pytest

import taudem_amd as T
from taudem_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPUTE = ("tdx_sinmapsi", "tdx_sinmapsi_dev", "tdx_sinmapsi_strip")


def _declarations():
    """symbol -> number of parameters, of the extension header"""
    text = open(os.path.join(ROOT, "include", "taudem_amd_sinmap.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(tdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_main_header_includes_the_extension():
    text = open(os.path.join(ROOT, "include", "taudem_amd.h")).read()
    assert '#include "taudem_amd_sinmap.h"' in text


def test_library_exports_every_declared_symbol_with_a_signature():
    lib, decl = T.load(), _declarations()
    assert set(decl) == set(COMPUTE) | {"tdx_sinmap_read_calpar", "tdx_tool_sinmapsi"} == set(_lib.SINMAP_SYMBOLS)
    for other in (_lib.EXPORTED_SYMBOLS, _lib.DROPAN_SYMBOLS, _lib.PEUKER_SYMBOLS, _lib.STREAMNET_SYMBOLS, _lib.OUTLETS_SYMBOLS):
        assert not set(decl) & set(other)
    for sym, nparams in decl.items():
        fn = getattr(lib, sym)
        assert fn.restype is _lib._SINMAP_SIGNATURES[sym][0] and len(fn.argtypes) == nparams, sym
    assert decl["tdx_sinmapsi"] == decl["tdx_sinmapsi_dev"] == decl["tdx_sinmapsi_strip"] - 1 == 26 and decl["tdx_tool_sinmapsi"] == 11


@pytest.mark.parametrize("sym", COMPUTE)
def test_null_context_is_a_bad_argument(sym):
    fn = getattr(T.load(), sym)
    rc = fn(*[t() for t in fn.argtypes])   # null context, null pointers, zeros
    assert rc == _lib.TDX_ERR_ARG
    assert _lib.last_error(None) == sym + ": bad argument"


def test_stage_methods_exist():
    from taudem_amd import tools
    from taudem_amd.distributed import StripPipeline

    assert callable(T.Context.sinmapsi) and callable(StripPipeline.sinmapsi) and callable(T.sinmapsi) and callable(tools.sinmapsi) and callable(T.read_calpar)
    assert callable(tools.sindexcombined)
    par = inspect.signature(T.Context.sinmapsi).parameters
    assert list(par)[:11] == ["self", "slp", "sca", "cal", "regions", "rminter", "rmaxter", "g", "rhow", "scamin", "scamax"]
    assert par["scamin"].default is None and par["scamax"].default is None and par["out"].default is None and par["stats"].default is False
    assert list(inspect.signature(StripPipeline.sinmapsi).parameters)[:11] == list(par)[:11]
    assert "sinmapsi" not in vars(T.Context) and "sinmapsi" not in vars(StripPipeline)   # mixins: the classes' own method sets are pinned
    assert list(inspect.signature(tools.sindexcombined).parameters) == ["slopefile", "scaterrainfile", "scarminroadfile", "scarmaxroadfile", "tergridfile", "terparfile",
                                                                        "satfile", "sincombinedfile", "Rminter", "Rmaxter", "par"]


def test_shim_forwards_sindexcombined():
    text = open(os.path.join(ROOT, "taudem_amd", "csrc", "integration", "taudem_amd_shim.cpp")).read()
    assert re.search(r"int sindexcombined\(char\* slopefile.*double Rminter, double Rmaxter, double\* par\)\s*\{ return tdx_tool_sinmapsi\(", text)


def test_regions_are_taken_as_table_rows_or_path(tmp_path):
    import numpy as np

    import sinmap_model as M
    from taudem_amd import api

    path = tmp_path / "calpar.csv"
    path.write_text(M.CALPAR)
    want = M.parse_calpar(M.CALPAR)
    rows = [tuple(want[k][i] for k in M.FIELDS) for i in range(4)]
    for given in (str(path), path, want, rows, T.read_calpar(str(path))):
        cols = api._regions(given)
        assert len(cols) == 8 and cols[0].dtype == np.int32 and all(c.dtype == np.float32 for c in cols[1:])
        assert all(np.array_equal(c, want[k]) for c, k in zip(cols, M.FIELDS))
    with pytest.raises(ValueError):
        api._regions([(1, 2.0, 3.0)])
