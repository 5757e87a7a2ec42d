"""The terrain-index part of the C ABI (include/taudem_amd_indices.h, which include/taudem_amd.h includes) held the way tests/test_sinmap_bindings.py holds the
SinmapSI header: the library exports every symbol it declares, taudem_amd/_lib.py has a ctypes signature with as many arguments as the declaration for each
and binds no other, none of them is in another table, and the nine compute forms reject a null context with TDX_ERR_ARG and their own "<symbol>: bad
argument" text before they touch HIP.  Context and StripPipeline have the stage methods as mixins; the shim forwards the five tool functions with the
reference's prototypes; the Makefile builds the five tools.  No GPU is needed."""
import inspect
import os
import re

import pytest

import taudem_amd as T
from taudem_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPUTE = tuple(f"tdx_{t}{form}" for t in ("terrain_indices", "lengtharea", "setregion") for form in ("", "_dev", "_strip"))
TOOLS = ("tdx_tool_twi", "tdx_tool_slopearea", "tdx_tool_slopearearatio", "tdx_tool_lengtharea", "tdx_tool_setregion")
STAGES = ("terrain_indices", "twi", "slopearea", "slopearearatio", "lengtharea", "setregion")


def _declarations():
    """symbol -> number of parameters, of the extension header"""
    text = open(os.path.join(ROOT, "include", "taudem_amd_indices.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(tdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_main_header_includes_the_extension():
    text = open(os.path.join(ROOT, "include", "taudem_amd.h")).read()
    assert '#include "taudem_amd_indices.h"' in text


def test_library_exports_every_declared_symbol_with_a_signature():
    lib, decl = T.load(), _declarations()
    assert set(decl) == set(COMPUTE) | set(TOOLS) == set(_lib.INDICES_SYMBOLS)
    for other in (_lib.EXPORTED_SYMBOLS, _lib.DROPAN_SYMBOLS, _lib.PEUKER_SYMBOLS, _lib.STREAMNET_SYMBOLS, _lib.OUTLETS_SYMBOLS, _lib.SINMAP_SYMBOLS):
        assert not set(decl) & set(other)
    for sym, nparams in decl.items():
        fn = getattr(lib, sym)
        assert fn.restype is _lib._INDICES_SIGNATURES[sym][0] and len(fn.argtypes) == nparams, sym
    assert decl["tdx_terrain_indices"] == decl["tdx_terrain_indices_dev"] == decl["tdx_terrain_indices_strip"] - 1 == 13
    assert decl["tdx_lengtharea"] == decl["tdx_lengtharea_dev"] == decl["tdx_lengtharea_strip"] - 1 == 9
    assert decl["tdx_setregion"] == decl["tdx_setregion_dev"] == decl["tdx_setregion_strip"] - 1 == 10
    assert [decl[t] for t in TOOLS] == [3, 4, 3, 4, 4]


@pytest.mark.parametrize("sym", COMPUTE)
def test_null_context_is_a_bad_argument(sym):
    fn = getattr(T.load(), sym)
    rc = fn(*[t() for t in fn.argtypes])   # null context, null pointers, zeros
    assert rc == _lib.TDX_ERR_ARG
    assert _lib.last_error(None) == sym + ": bad argument"


@pytest.mark.parametrize("sym", TOOLS)
def test_tool_functions_refuse_null_names(sym):
    fn = getattr(T.load(), sym)
    assert fn(*[t() for t in fn.argtypes]) == _lib.TDX_ERR_ARG and _lib.last_error(None) == sym + ": bad argument"


def test_stage_methods_exist():
    from taudem_amd import tools
    from taudem_amd.distributed import StripPipeline

    for name in STAGES:
        assert callable(getattr(T.Context, name)) and callable(getattr(StripPipeline, name))
        assert name not in vars(T.Context) and name not in vars(StripPipeline)   # mixins: the classes' own method sets are pinned
    assert callable(T.terrain_indices) and callable(T.lengtharea) and callable(T.setregion)
    par = inspect.signature(T.Context.terrain_indices).parameters
    assert list(par)[:6] == ["self", "slp", "sca", "m", "n", "want"] and par["want"].default == ("twi", "sa", "sar") and par["m"].default == 2.0 and par["n"].default == 1.0
    assert par["out"].default is None and par["stats"].default is False
    assert list(inspect.signature(StripPipeline.terrain_indices).parameters)[:6] == list(par)[:6]
    par = inspect.signature(T.Context.lengtharea).parameters
    assert list(par)[:5] == ["self", "plen", "ad8", "M", "y"] and abs(par["M"].default - 0.03) < 1e-12 and abs(par["y"].default - 1.3) < 1e-12
    par = inspect.signature(T.Context.setregion).parameters
    assert list(par)[:4] == ["self", "p", "gw", "region_id"] and par["region_id"].default == 1
    # the reference's names and argument lists
    assert list(inspect.signature(tools.twigrid).parameters) == ["slopefile", "areafile", "twifile"]
    assert list(inspect.signature(tools.slopearea).parameters) == ["slopefile", "scafile", "safile", "p"]
    assert list(inspect.signature(tools.atanbgrid).parameters) == ["slopefile", "areafile", "atanbfile"]
    assert list(inspect.signature(tools.lengtharea).parameters) == ["plenfile", "ad8file", "ssfile", "p"]
    assert list(inspect.signature(tools.setregion).parameters) == ["fdrfile", "regiongwfile", "newfile", "regionID"]


def test_want_is_checked_before_the_library_is_entered():
    from taudem_amd import api

    class Frame:   # no raster is looked at before `want` has been
        def raster(self, *a):
            raise AssertionError("want was not checked first")

    for want in ((), ("twi", "twi"), ("si",), ("twi", "sa", "sar", "twi")):
        with pytest.raises(ValueError):
            api._terrain_indices(Frame(), None, None, 2.0, 1.0, want, -1.0, -1.0, None)


def test_shim_forwards_the_five_tool_functions():
    text = open(os.path.join(ROOT, "taudem_amd", "csrc", "integration", "taudem_amd_shim.cpp")).read()
    for proto, target in ((r"int twigrid\(char\* slopefile, char\* areafile, char\* twifile\)", "tdx_tool_twi"),
                          (r"int slopearea\(char\* slopefile, char\* scafile, char\* safile, float\* p\)", "tdx_tool_slopearea"),
                          (r"int atanbgrid\(char\* slopefile, char\* areafile, char\* atanbfile\)", "tdx_tool_slopearearatio"),
                          (r"int lengtharea\(char\* plenfile, char\* ad8file, char\* ssfile, float\* p\)", "tdx_tool_lengtharea"),
                          (r"int setregion\(char\* fdrfile, char\* regiongwfile, char\* newfile, int32_t regionID\)", "tdx_tool_setregion")):
        assert re.search(proto + r"\s*\{ return " + target + r"\(", text), target


def test_makefile_builds_the_five_tools_and_the_kernels():
    text = open(os.path.join(ROOT, "taudem_amd", "csrc", "Makefile")).read()
    tools_line = next(line for line in text.splitlines() if line.startswith("TOOLS"))
    for t in ("twi", "slopearea", "slopearearatio", "lengtharea", "setregion"):
        assert f" {t}" in tools_line and os.path.exists(os.path.join(ROOT, "taudem_amd", "csrc", "tools", t + ".cpp"))
        assert os.access(os.path.join(ROOT, "taudem_amd", "bin", t), os.X_OK)
    assert " indices.hip" in next(line for line in text.splitlines() if line.startswith("HIPSRC"))
