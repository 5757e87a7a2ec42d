"""The StreamNet part of the C ABI (include/taudem_amd_streamnet.h, which include/taudem_amd.h includes) held the way tests/test_dropan_bindings.py holds
DropAnalysis': the library exports every symbol the header declares, taudem_amd/_lib.py has a ctypes signature with as many arguments as the declaration
for each and binds no other, and the compute forms reject a null context with TDX_ERR_ARG and their own "<symbol>: bad argument" text before they touch
HIP.  Context has the stage method, tools has netsetup, and the tool function refuses the network layer before it reads anything.  No GPU is needed."""
import os
import re

import pytest

import taudem_amd as T
from taudem_amd import _lib, tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPUTE = ("tdx_streamnet", "tdx_streamnet_dev", "tdx_streamnet_compact_strip", "tdx_streamnet_label_strip", "tdx_streamnet_links_build")


def _declarations():
    """symbol -> number of parameters, of the extension header"""
    text = open(os.path.join(ROOT, "include", "taudem_amd_streamnet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(tdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_main_header_includes_the_extension():
    text = open(os.path.join(ROOT, "include", "taudem_amd.h")).read()
    assert '#include "taudem_amd_streamnet.h"' in text


def test_library_exports_every_declared_symbol_with_a_signature():
    lib, decl = T.load(), _declarations()
    assert set(decl) == set(_lib.STREAMNET_SYMBOLS) and set(COMPUTE) <= set(decl) and "tdx_tool_streamnet" in decl
    assert not set(decl) & set(_lib.EXPORTED_SYMBOLS)
    for sym, nparams in decl.items():
        fn = getattr(lib, sym)
        assert fn.restype is _lib._STREAMNET_SIGNATURES[sym][0] and len(fn.argtypes) == nparams, sym


@pytest.mark.parametrize("sym", COMPUTE)
def test_null_context_is_a_bad_argument(sym):
    fn = getattr(T.load(), sym)
    rc = fn(*[t() for t in fn.argtypes])   # null context, null pointers, zeros
    assert rc == _lib.TDX_ERR_ARG
    assert _lib.last_error(None) == sym + ": bad argument"


def test_links_accessors_take_a_null_handle():
    lib = T.load()
    assert lib.tdx_streamnet_links_count(None, None, None) == 0
    lib.tdx_streamnet_links_copy(None, None, None, None)
    lib.tdx_streamnet_links_free(None)
    assert lib.tdx_streamnet_compact_count(None) == 0
    lib.tdx_streamnet_compact_free(None)
    assert lib.tdx_streamnet_write_text(None, b"t", b"c") == _lib.TDX_ERR_ARG


def test_network_layer_is_refused_before_anything_is_read(tmp_path, capfd):
    missing = str(tmp_path / "missing.tif")
    rc = tools.netsetup(missing, missing, missing, missing, missing, str(tmp_path / "tree.txt"), str(tmp_path / "coord.txt"), wfile=missing,
                        streamnetsrc=str(tmp_path / "net.shp"))
    out = capfd.readouterr()
    assert rc == _lib.TDX_ERR_ARG and "-net" in out.err and "StreamNet version" not in out.out and not os.listdir(tmp_path)


def test_stage_methods_exist():
    from taudem_amd.distributed import StripPipeline

    assert callable(StripPipeline.streamnet_compact) and callable(StripPipeline.streamnet_label) and callable(T.StreamNetLinks)
    assert callable(T.Context.streamnet) and callable(T.streamnet) and callable(T.streamnet_text) and callable(tools.netsetup) and tools.streamnet is tools.netsetup
    assert T.streamnet_text([[3, 0, 1, -1, 1, 2, 2, -1, 4]], [[1.5, 2.0, 0.0, 10.25, 900.0]]) == (b"\t3\t0\t1\t-1\t1\t2\t2\t-1\t4\n",
                                                                                                  b"\t1.500000\t2.000000\t0.000000\t10.250000\t900.000000\n")
