"""tdx_streamnet_net_rows (taudem_amd.streamnet_net) on rows parsed from the committed -tree / -coord text of tests/golden/streamnet_*.npz: equal to
tests/netlayer_model.net_rows on the same rows, bit for bit, on every case and hand-built raster; equal to the reference's record wherever the generator
stored that the text reproduces it (exact_<v> - four projected cases qualify) and, with the record's vertices in place of the text's, on the geographic
case too.  A link of a single point - no reference run produces one, its -coord rows hold a one-cell link's cell twice - is a line of ONE vertex.  Rows
that point outside coord are refused.  No GPU is needed."""
import subprocess
import os

import numpy as np
import pytest

import netlayer_model as N
import streamnet_model as M
import taudem_amd as T
from taudem_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [str(n) for n in N.load("small")["names"]]
RUNS = [(name, "") for name in M.CASES] + [("small", n + "_") for n in SMALL]


def _lib_layer(tree, coord, geographic):
    fields, lines = T.streamnet_net(tree, coord, geographic)
    assert list(fields) == list(N.FIELDS) and all(fields[k].dtype == (np.int32 if k in N.INT_FIELDS else np.float64) for k in fields)
    return {k: v.tolist() for k, v in fields.items()}, lines


@pytest.mark.parametrize("name,prefix", RUNS)
def test_rows_equal_the_model_and_the_record(name, prefix):
    rec, fix = N.load(name), M.load_golden(name)
    geographic = name == "geographic"
    qualified = 0
    for v in N.VARIANTS:
        tree, coord = N.rows_of_text(fix[f"{prefix}tree_{v}"], fix[f"{prefix}coord_{v}"])
        got = _lib_layer(tree, coord, geographic)
        if not len(tree):
            assert got[1] == []
            continue
        assert N.same_layer(got, N.net_rows(tree, coord, geographic)), (name, prefix, v)
        want = N.parse_lines(N.text(rec[f"{prefix}net_{v}"]))
        if bool(rec[f"{prefix}exact_{v}"]):
            assert N.same_layer(got, want), (name, prefix, v)
            qualified += 1
        for t, ln in zip(tree, want[1]):
            coord[t[1]:t[2] + 1, :2] = ln[::-1]
        assert N.same_layer(_lib_layer(tree, coord, geographic), want), (name, prefix, v)
    assert qualified == 2 or geographic or name == "small"


def test_a_link_of_one_point_is_a_line_of_one_vertex():
    tree = np.array([[0, 0, 0, -1, 1, -1, 2, -1, 2], [1, 1, 3, 0, -1, -1, 1, 7, 1], [2, 4, 5, 0, -1, -1, 1, -1, 1]], np.int64)
    coord = np.array([[5, 5, 0, 10, 900], [1, 9, 50.5, 14.25, 100], [1, 8, 40, 13, 200], [5, 5, 0, 10, 900], [3, 3, 7, 11, 50], [3, 3, 7, 11, 60]], np.float64)
    for geographic in (False, True):
        fields, lines = _lib_layer(tree, coord, geographic)
        assert [len(ln) for ln in lines] == [1, 3, 2] and lines[1].tolist() == [[5, 5], [1, 8], [1, 9]]   # reversed: vertex 0 is the downstream end
        assert N.same_layer((fields, lines), N.net_rows(tree, coord, geographic))
        assert fields["Length"][0] == 0 and fields["Slope"][0] == 0 and fields["StraightL"][0] == 0 and fields["DSContArea"][0] == 900
        assert fields["Length"][2] == 0 and fields["Slope"][2] == 0 and fields["DSContArea"][2] == 50   # two points on one spot: nothing moved
        assert fields["strmDrop"][1] == 4.25 and fields["DOUTEND"][1] == 0 and fields["DOUTSTART"][1] == 50.5 and fields["DOUTMID"][1] == 25.25
        assert fields["USContArea"][1] == 100 and fields["DSContArea"][1] == 200 and fields["DSNODEID"] == [-1, 7, -1] and fields["WSNO"] == fields["LINKNO"] == [0, 1, 2]
    assert _lib_layer(tree, coord, False)[0]["Length"][1] == 1 + 5 and _lib_layer(tree, coord, False)[0]["StraightL"][1] == np.sqrt(32.0)


def test_refusals_and_the_written_layer(tmp_path):
    lib = T.load()
    tree = np.array([[0, 0, 2, -1, -1, -1, 1, -1, 1]], np.int64)
    coord = np.zeros((2, 5))
    out = [np.zeros(9), np.zeros(2, np.int64), np.zeros(3), np.zeros(3)]
    rc = lib.tdx_streamnet_net_rows(tree.ctypes.data, coord.ctypes.data, 1, 2, 0, 3, *[a.ctypes.data for a in out])
    assert rc == _lib.TDX_ERR_ARG and "not in coord" in _lib.last_error(None)
    tree[0, 2] = 1
    rc = lib.tdx_streamnet_net_rows(tree.ctypes.data, coord.ctypes.data, 1, 2, 0, 3, *[a.ctypes.data for a in out])
    assert rc == _lib.TDX_ERR_ARG and "2 vertices, not 3" in _lib.last_error(None)
    assert lib.tdx_streamnet_net_rows(None, None, 1, 0, 0, 0, None, None, None, None) == _lib.TDX_ERR_ARG
    assert lib.tdx_streamnet_net_write(None, 0, b"x.shp") == _lib.TDX_ERR_ARG
    # write_lines with the reference's widths: the .dbf columns of the -net layer
    fix = M.load_golden("plain")
    t, c = N.rows_of_text(fix["tree_plain"], fix["coord_plain"])
    fields, lines = T.streamnet_net(t, c)
    T.write_lines(str(tmp_path / "net.shp"), lines, fields, T.api.NET_WIDTHS)
    import vector_parse as V
    d = V.dbf(str(tmp_path / "net.dbf"))
    assert [(f[0], f[2], f[3]) for f in d["fields"]] == [(n, w, dec) for n, _, w, dec in _lib.NET_FIELDS] and d["nrecords"] == len(t)


def test_stand_alone_program(tmp_path):
    """tests/netlayer/netlayer_main.cpp: the host files without the library (the program that runs under the sanitizers)"""
    exe = str(tmp_path / "netlayer_main")
    src = [os.path.join(ROOT, "tests", "netlayer", "netlayer_main.cpp")] + [os.path.join(ROOT, "taudem_amd", "csrc", f) for f in ("vector_layer.cpp", "streamnet_net.cpp", "catchoutlets.cpp")]
    subprocess.run(["c++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "taudem_amd", "csrc")] + src + ["-o", exe], check=True)
    r = subprocess.run([exe, "roundtrip", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
    assert subprocess.run([exe, "net"], capture_output=True, text=True).stdout == "1 3 0 6 17\nrefused\n"
    r = subprocess.run([exe, "chain", "20000"], capture_output=True, text=True)   # no recursion: a chain of any length is walked
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "20000 20000" and "cycle" in r.stdout.splitlines()[1], r.stdout + r.stderr
