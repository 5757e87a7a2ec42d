"""The PeukerDouglas part of the C ABI (include/taudem_amd_peuker.h, which include/taudem_amd.h includes) held the way tests/test_dropan_bindings.py
holds the DropAnalysis header: the library exports every symbol it declares, taudem_amd/_lib.py has a ctypes signature with as many arguments as the
declaration for each and binds no other, none of them is in the main table, and the three compute forms reject a null context with TDX_ERR_ARG and
their own "<symbol>: bad argument" text before they touch HIP.  Context and StripPipeline have the stage method.  No GPU is needed."""
import inspect
import os
import re

import pytest

import taudem_amd as T
from taudem_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPUTE = ("tdx_peukerdouglas", "tdx_peukerdouglas_dev", "tdx_peukerdouglas_strip")


def _declarations():
    """symbol -> number of parameters, of the extension header"""
    text = open(os.path.join(ROOT, "include", "taudem_amd_peuker.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(tdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_main_header_includes_the_extension():
    text = open(os.path.join(ROOT, "include", "taudem_amd.h")).read()
    assert '#include "taudem_amd_peuker.h"' in text


def test_library_exports_every_declared_symbol_with_a_signature():
    lib, decl = T.load(), _declarations()
    assert set(decl) == set(COMPUTE) | {"tdx_tool_peukerdouglas"} == set(_lib.PEUKER_SYMBOLS)
    assert not set(decl) & set(_lib.EXPORTED_SYMBOLS) and not set(decl) & set(_lib.DROPAN_SYMBOLS)
    for sym, nparams in decl.items():
        fn = getattr(lib, sym)
        assert fn.restype is _lib._PEUKER_SIGNATURES[sym][0] and len(fn.argtypes) == nparams, sym


@pytest.mark.parametrize("sym", COMPUTE)
def test_null_context_is_a_bad_argument(sym):
    fn = getattr(T.load(), sym)
    rc = fn(*[t() for t in fn.argtypes])   # null context, null pointers, zeros
    assert rc == _lib.TDX_ERR_ARG
    assert _lib.last_error(None) == sym + ": bad argument"


def test_stage_methods_exist():
    from taudem_amd import tools
    from taudem_amd.distributed import StripPipeline

    assert callable(T.Context.peukerdouglas) and callable(StripPipeline.peukerdouglas) and callable(T.peukerdouglas) and callable(tools.peukerdouglas)
    par = inspect.signature(T.Context.peukerdouglas).parameters
    assert list(par) == ["self", "fel", "nodata", "weights", "float_weights", "out", "stats"] and par["weights"].default == (0.4, 0.1, 0.05)
    assert "peukerdouglas" not in vars(T.Context) and "peukerdouglas" not in vars(StripPipeline)   # mixins: the classes' own method sets are pinned
