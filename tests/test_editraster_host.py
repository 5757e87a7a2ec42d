"""EditRaster without a GPU: the header (include/taudem_amd_editraster.h, which include/taudem_amd.h includes) held the way tests/test_indices_bindings.py holds
the terrain-index header; the change-file reader (tdx_editraster_read_changes, taudem_amd.read_changes) against the Python restatement of the scanner on the
change files of tests/golden/editraster_small.npz, with the value no int16 holds refused; the numpy model against the real tool's recorded rasters; the
refusals that precede any HIP call; and the error transcripts of bin/editraster."""
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import editraster_model as M
import taudem_amd as T
from taudem_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "editraster_small.npz"))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tool_transcripts_editraster.json")
COMPUTE = ("tdx_editraster", "tdx_editraster_dev", "tdx_editraster_strip")
RUNS = [(c, f) for c, (_, _, files) in M.cases().items() for f in files]


def _declarations():
    text = open(os.path.join(ROOT, "include", "taudem_amd_editraster.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(tdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_header_library_and_signatures_agree():
    assert '#include "taudem_amd_editraster.h"' in open(os.path.join(ROOT, "include", "taudem_amd.h")).read()
    lib, decl = T.load(), _declarations()
    assert set(decl) == set(COMPUTE) | {"tdx_editraster_read_changes", "tdx_tool_editraster"} == set(_lib.EDITRASTER_SYMBOLS)
    for other in (_lib.EXPORTED_SYMBOLS, _lib.DROPAN_SYMBOLS, _lib.PEUKER_SYMBOLS, _lib.STREAMNET_SYMBOLS, _lib.OUTLETS_SYMBOLS, _lib.SINMAP_SYMBOLS, _lib.INDICES_SYMBOLS):
        assert not set(decl) & set(other)
    for sym, nparams in decl.items():
        fn = getattr(lib, sym)
        assert fn.restype is _lib._EDITRASTER_SIGNATURES[sym][0] and len(fn.argtypes) == nparams, sym
    assert decl["tdx_editraster"] == decl["tdx_editraster_dev"] == decl["tdx_editraster_strip"] - 2 == 11   # the strip form: comm and row0
    assert decl["tdx_tool_editraster"] == 3


@pytest.mark.parametrize("sym", COMPUTE + ("tdx_editraster_read_changes", "tdx_tool_editraster"))
def test_null_arguments_are_a_bad_argument(sym):
    fn = getattr(T.load(), sym)
    assert fn(*[t() for t in fn.argtypes]) == _lib.TDX_ERR_ARG and _lib.last_error(None) == sym + ": bad argument"


def test_stage_methods_tool_shim_and_makefile():
    from taudem_amd import tools
    from taudem_amd.distributed import StripPipeline

    assert callable(T.Context.editraster) and callable(StripPipeline.editraster) and callable(T.editraster) and callable(T.read_changes)
    assert "editraster" not in vars(T.Context) and "editraster" not in vars(StripPipeline)   # mixins: the classes' own method sets are pinned
    par = inspect.signature(T.Context.editraster).parameters
    assert list(par)[:6] == ["self", "raster", "cols", "rows", "vals", "out"] and par["out"].default is None and par["stats"].default is False
    assert list(inspect.signature(StripPipeline.editraster).parameters)[:6] == ["self", "raster", "cols", "rows", "vals", "row0"]
    assert list(inspect.signature(tools.editraster).parameters) == ["rasterfile", "newfile", "changefile"]   # src/EditRaster.cpp:69
    shim = open(os.path.join(ROOT, "taudem_amd", "csrc", "integration", "taudem_amd_shim.cpp")).read()
    assert re.search(r"int editraster\(char\* rasterfile, char\* newfile, char\* changefile\)\s*\{ return tdx_tool_editraster\(", shim)
    mk = open(os.path.join(ROOT, "taudem_amd", "csrc", "Makefile")).read()
    assert " editraster" in next(ln for ln in mk.splitlines() if ln.startswith("TOOLS")) and " editraster.hip" in next(ln for ln in mk.splitlines() if ln.startswith("HIPSRC"))
    assert os.access(os.path.join(ROOT, "taudem_amd", "bin", "editraster"), os.X_OK)


@pytest.mark.parametrize("case,fname", RUNS)
def test_reader_equals_the_restated_scanner(case, fname, tmp_path):
    text = str(GOLD[f"changes/{case}/{fname}"])
    assert text == M.cases()[case][2][fname]   # the fixture holds the model's files
    path = tmp_path / "changes.txt"
    path.write_text(text)
    x, y, v = T.read_changes(str(path))
    ex, ey, ev = M.scan_changes(text)
    assert v.dtype == np.int32 and np.array_equal(x, ex) and np.array_equal(y, ey) and np.array_equal(v, ev)
    assert len(v) == {"none": 0, "dup": 3, "edges": 6, "malformed": 1, "values": 3}[fname]


@pytest.mark.parametrize("case,fname", RUNS)
def test_model_equals_the_reference_record(case, fname):
    a, nodata = GOLD[f"in/{case}"], int(GOLD[f"nodata/{case}"])
    gt = M.geotransform(a.shape[0])
    x, y, v = M.scan_changes(str(GOLD[f"changes/{case}/{fname}"]))
    c, r = M.cells(x, y, gt)
    assert np.array_equal(M.edit(a, nodata, c, r, v), GOLD[f"out/{case}/{fname}"])
    lines = [ln for ln in str(GOLD[f"stdout/{case}/{fname}"]).splitlines() if ln.startswith("Process:")]
    assert lines == M.process_lines(x, y, v, gt, a.shape, as_reference=True)


def test_reader_edge_cases(tmp_path):
    lib = T.load()
    n = np.zeros(1, np.int64)

    def read(text, cap=8):
        p = tmp_path / "c.txt"
        p.write_text(text)
        x, y, v = np.full(cap, -7.0), np.full(cap, -7.0), np.full(cap, -7, np.int32)
        rc = lib.tdx_editraster_read_changes(str(p).encode(), cap, x.ctypes.data, y.ctypes.data, v.ctypes.data, n.ctypes.data)
        return rc, int(n[0]), x, y, v

    assert read("")[:2] == (0, 0) and read("no newline at all")[:2] == (0, 0) and read("h\n\n\n")[:2] == (0, 0)
    rc, k, x, y, v = read("1.5,2.5,3\n4,5,6\n")   # the first line is the header, whatever it holds
    assert (rc, k) == (0, 1) and (x[0], y[0], v[0]) == (4.0, 5.0, 6)
    rc, k, x, y, v = read("h\n1,2,3 4,5,6\n7,8,9x\n10,11,12\n")   # records need no line of their own; "x" ends the scan
    assert (rc, k) == (0, 3) and list(v[:3]) == [3, 6, 9]
    rc, k, x, y, v = read("h\n1e2,-2.5E-1,+7\n1,2,3.5\n4,5,6\n")   # "3.5": 3 is taken, ".5\n4" scans as a number and the comma is missing
    assert (rc, k) == (0, 2) and (x[0], y[0], v[0]) == (100.0, -0.25, 7) and v[1] == 3
    assert read("h\n1,2,-32768\n1,2,32767\n")[:2] == (0, 2)
    for bad in ("32768", "-32769", "99999999999999999999"):
        rc, k, x, y, v = read("h\n1,2,5\n1,2,%s\n1,2,6\n" % bad)
        assert rc == _lib.TDX_ERR_ARG and k == 1 and v[0] == 5 and v[1] == -7 and "outside -32768 .. 32767" in _lib.last_error(None)
    rc, k, x, y, v = read("h\n1,2,3\n4,5,6\n7,8,9\n", cap=2)   # the count is the file's, the first `capacity` records are stored
    assert (rc, k) == (0, 3) and list(v) == [3, 6]
    assert lib.tdx_editraster_read_changes(str(tmp_path / "nope.txt").encode(), 0, None, None, None, n.ctypes.data) == _lib.TDX_ERR_FILE
    with pytest.raises(_lib.TdxError) as e:
        (tmp_path / "big.txt").write_text("h\n1,2,40000\n")
        T.read_changes(str(tmp_path / "big.txt"))
    assert e.value.code == _lib.TDX_ERR_ARG
    long_header = "x" * 5000 + "\n1,2,3\n"   # readline() stops after MAXLN = 4096 characters: the rest of the line is scanned, and does not scan
    assert read(long_header)[:2] == (0, 0)


@pytest.fixture(scope="module")
def changes_main(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("changes_main") / "changes_main")
    src = [os.path.join(ROOT, "tests", "editraster", "changes_main.cpp"), os.path.join(ROOT, "taudem_amd", "csrc", "editraster_changes.cpp")]
    subprocess.run(["c++", "-O1", "-g", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "taudem_amd", "csrc")] + src + ["-o", exe], check=True)
    return exe


def _select(exe, cols, rows, vals, nx, lo, hi):
    text = "".join(f"{c} {r} {v}\n" for c, r, v in zip(cols, rows, vals))
    r = subprocess.run([exe, "select", str(nx), str(lo), str(hi)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if r.stdout == "refused\n":
        return None
    return [tuple(int(w) for w in ln.split()) for ln in r.stdout.splitlines()]


def test_selection_keeps_the_last_change_of_a_cell(changes_main):
    """What the device scatters: per cell of the owned rows the LAST change of the list, cells ascending and relative to the first owned row; changes off the
    raster or in another strip's rows dropped; a value no int16 holds - wherever its cell lies - refuses the whole list."""
    rng = np.random.default_rng(99)
    nx, ny, n = 7, 9, 400
    cols, rows, vals = rng.integers(-2, nx + 2, n), rng.integers(-2, ny + 2, n), rng.integers(-32768, 32768, n)
    for lo, hi in ((0, ny), (0, 1), (3, 6), (8, 9), (4, 4)):
        want = {}
        for c, r, v in zip(cols, rows, vals):
            if 0 <= c < nx and lo <= r < hi:
                want[(r - lo) * nx + c] = int(v)
        got = _select(changes_main, cols, rows, vals, nx, lo, hi)
        assert got == sorted(want.items()) and (len(got) > 0) == (hi > lo)
    assert _select(changes_main, [], [], [], nx, 0, ny) == []
    assert _select(changes_main, [0, 1, 0], [0, 0, 0], [5, 6, 7], nx, 0, ny) == [(0, 7), (1, 6)]
    for bad in (32768, -32769, 2 ** 31 - 1):
        assert _select(changes_main, [0, 99], [0, 99], [1, bad], nx, 0, ny) is None    # the offender lies off the raster
        assert _select(changes_main, [0, 0], [0, 0], [bad, 1], nx, 0, ny) is None      # or is overwritten later


def test_stand_alone_reader_equals_the_library(changes_main, tmp_path):
    for case, fname in RUNS:
        p = tmp_path / f"{case}_{fname}.txt"
        p.write_text(str(GOLD[f"changes/{case}/{fname}"]))
        out = subprocess.run([changes_main, "read", str(p)], capture_output=True, text=True, check=True).stdout.splitlines()
        x, y, v = T.read_changes(str(p))
        assert out[0] == f"0 {len(v)}" and [tuple(float(w) for w in ln.split()) for ln in out[1:]] == list(zip(x, y, v))
    assert subprocess.run([changes_main, "read", str(tmp_path / "nope")], capture_output=True, text=True).stdout == "1 0\n"
    (tmp_path / "big.txt").write_text("h\n1,2,3\n1,2,32768\n")
    assert subprocess.run([changes_main, "read", str(tmp_path / "big.txt")], capture_output=True, text=True).stdout.splitlines()[0] == "2 1"


def test_error_runs_reproduce_the_recorded_transcripts():
    spec = importlib.util.spec_from_file_location("editraster_transcripts", os.path.join(ROOT, "scripts", "editraster_transcripts.py"))
    et = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(et)
    expected = et.load_fixture(FIXTURE, "err")
    assert len(expected) == 3 and all(not any(e["files"].values()) for e in expected.values())   # no run leaves a file
    e = expected["err/editraster/missing_raster"]          # the ToolRun frame's status for a file it cannot read (TDX_ERR_FILE)
    assert e["status"] == 21 and e["stdout"].startswith("Editraster version ") and "Error opening file" in e["stdout"]
    e = expected["err/editraster/missing_changes"]
    assert e["status"] == 21 and e["stdout"].endswith("Error opening file $D/wide/nope.txt.\n") and e["stderr"] == "Time estimate not available.\n"
    e = expected["err/editraster/value_outside_int16"]     # the reference's main's words for a non-zero code (src/EditRastermn.cpp:91-92), exit status 0
    assert e["status"] == 0 and e["stdout"].endswith("Threshold Error -1\n") and "record 1 of" in e["stderr"] and "Process:" not in e["stdout"]
    bad = et.differences(expected, et.collect("err"))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("args", [[], ["-in"], ["-in", "a.tif", "-out", "b.tif", "-changes"], ["-in", "a.tif", "-o", "b.tif"], ["a.tif"]])
def test_usage_is_the_reference_s(args):
    """src/EditRastermn.cpp:54,95-99: fewer than two words, a flag without a value or an unknown flag print the usage and end with status 0"""
    exe = os.path.join(ROOT, "taudem_amd", "bin", "editraster")
    p = subprocess.run([exe, *args], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == ""
    assert p.stdout == f"Editraster use:\n {exe} -in <filetochange>\n-out <filetowrite> \n-changes <file with change values (x,y,newvalue)> \n"
