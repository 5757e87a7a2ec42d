"""The surface of the device link builder without a GPU: the new symbols are declared in include/taudem_amd_streamnet.h, exported by the library and
bound with the header's parameter counts; the compute forms refuse null arguments with their own words; where the links are built is a word, "host" or
"device", everywhere, and any other word is refused before a device is touched; the command-line tool refuses another word with exit status 2 before
anything is read."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import taudem_amd as T
from taudem_amd import _lib, tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "taudem_amd", "bin", "streamnet")
NEW = {"tdx_streamnet_gpu_links": 23, "tdx_streamnet_gpu_links_dev": 23, "tdx_streamnet_links_build_gpu": 13, "tdx_streamnet_links_device_phases": 5,
       "tdx_tool_set_streamnet_links": 1}


def test_symbols_are_declared_exported_and_bound():
    h = open(os.path.join(ROOT, "include", "taudem_amd_streamnet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    decl = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(tdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}
    lib = T.load()
    for sym, nparams in NEW.items():
        assert decl.get(sym) == nparams and sym in _lib.STREAMNET_SYMBOLS and len(getattr(lib, sym).argtypes) == nparams, sym
    assert decl["tdx_streamnet_gpu_links"] == decl["tdx_streamnet"] and decl["tdx_streamnet_gpu_links_dev"] == decl["tdx_streamnet_dev"]
    assert decl["tdx_streamnet_links_build_gpu"] == decl["tdx_streamnet_links_build"] + 1
    for sym in ("tdx_streamnet_gpu_links", "tdx_streamnet_gpu_links_dev", "tdx_streamnet_links_build_gpu"):
        fn = getattr(lib, sym)
        assert fn(*[t() for t in fn.argtypes]) == _lib.TDX_ERR_ARG and _lib.last_error(None) == sym + ": bad argument", sym
    ms, a, b, c = np.full(len(_lib.STREAMNET_LINK_PHASES), 7.0), C.c_int64(5), C.c_int64(5), C.c_int64(5)
    assert lib.tdx_streamnet_links_device_phases(None, ms.ctypes.data_as(C.c_void_p), C.byref(a), C.byref(b), C.byref(c)) == 0
    for k, name in enumerate(_lib.STREAMNET_LINK_PHASES):
        assert re.search(rf"#define TDX_STREAMNET_DLINK_{name.upper()} {k}\b", h)
    assert f"#define TDX_STREAMNET_DLINK_PHASES {len(_lib.STREAMNET_LINK_PHASES)}" in h and "#define TDX_STREAMNET_PHASES 7" in h
    mk = open(os.path.join(ROOT, "taudem_amd", "csrc", "Makefile")).read()
    assert " streamnet_links_device.hip" in next(ln for ln in mk.splitlines() if ln.startswith("HIPSRC"))


def test_the_words():
    assert _lib.STREAMNET_LINKS == ("host", "device")
    lib = T.load()
    assert lib.tdx_tool_set_streamnet_links(2) == _lib.TDX_ERR_ARG and lib.tdx_tool_set_streamnet_links(-1) == _lib.TDX_ERR_ARG
    assert lib.tdx_tool_set_streamnet_links(1) == 0 and lib.tdx_tool_set_streamnet_links(0) == 0
    assert tools.set_streamnet_links("device") == 0 and tools.set_streamnet_links("host") == 0 and tools.set_streamnet_links() == 0
    with pytest.raises(ValueError):
        tools.set_streamnet_links("x")
    par = inspect.signature(T.Context.streamnet).parameters
    assert par["links"].default == "host" and par["links"].kind is inspect.Parameter.KEYWORD_ONLY
    par = inspect.signature(T.StreamNetLinks.__init__).parameters
    assert list(par)[-2:] == ["links", "ctx"] and par["links"].default == "host" and par["ctx"].default is None
    with pytest.raises(ValueError, match="elsewhere"):
        T.StreamNetLinks([], 3, 3, 1.0, 1.0, links="elsewhere")
    with pytest.raises(ValueError, match="ctx"):
        T.StreamNetLinks([], 3, 3, 1.0, 1.0, links="device")


def test_tool_refuses_another_word_before_anything_is_read(tmp_path):
    r = subprocess.run([EXE, "-links", "nonsense", "-p", str(tmp_path / "p.tif"), "-src", str(tmp_path / "src.tif"), "-fel", str(tmp_path / "fel.tif"), "-ad8",
                        str(tmp_path / "ad8.tif"), "-ord", str(tmp_path / "ord.tif"), "-w", str(tmp_path / "w.tif"), "-tree", str(tmp_path / "tree.txt"), "-coord",
                        str(tmp_path / "coord.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "host or device" in r.stderr and r.stdout == "" and not os.listdir(tmp_path)
