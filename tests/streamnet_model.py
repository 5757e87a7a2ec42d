"""StreamNet's semantics as a plain C++ program (tests/streamnet/streamnet_restate.cpp): whole-raster grids and literal FIFO queues, one rank.

    compile(dirpath)                       builds the shared library with `c++` into dirpath and returns a Restatement
    Restatement.run(p, src, fel, ad8, ...) -> (ord int16, w int32, tree int64 (n, 9), coord float64 (m, 5))
    tree_text(tree) / coord_text(coord)    the -tree / -coord files' bytes (src/streamnet.cpp:1165, :1177)
    inputs(case) / outlets_for(...)        the inputs of the golden runs (shared with tests/golden/make_golden_streamnet.py)
    small_rasters()                        the hand-built rasters

tests/test_streamnet_restatement.py holds it to every golden of tests/golden/streamnet_*.npz, so that the GPU tests can use it at sizes the
goldens do not cover.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "streamnet", "streamnet_restate.cpp")
P_NODATA = -32768
SRC_NODATA = -32768
W_NODATA = -2147483647
ORD_NODATA = -32768
CASES = ("plain", "holes", "rect_dxdy", "geographic", "fourway_mask")
THRESH = {"plain": 30, "holes": 30, "rect_dxdy": 25, "geographic": 35, "fourway_mask": 30}   # src = ad8 >= THRESH[case]
VARIANTS = ("plain", "outlets", "sw")
DX_ = (0, 1, 1, 0, -1, -1, -1, 0, 1)
DY_ = (0, 0, -1, -1, -1, 0, 1, 1, 1)


def tree_text(tree):
    return "".join("\t" + "\t".join(str(int(v)) for v in row) + "\n" for row in np.asarray(tree, np.int64).reshape(-1, 9))


def coord_text(coord):
    return "".join("\t%f\t%f\t%f\t%f\t%f\n" % tuple(float(v) for v in row) for row in np.asarray(coord, np.float64).reshape(-1, 5))


def gt4(gt):
    """{left edge, cell width, top edge, cell height} of a GDAL geotransform (src/tiffIO.cpp:96-99)."""
    return np.array([gt[0], abs(gt[1]), gt[3], abs(gt[5])], np.float64)


class Restatement:
    def __init__(self, lib_path):
        self._lib = C.CDLL(lib_path)
        P = C.c_void_p
        self._lib.sn_run.restype = C.c_int
        self._lib.sn_run.argtypes = [C.c_int, C.c_int, P, C.c_int16, P, C.c_int32, P, P, P, P, C.c_double, C.c_double, P, C.c_int, P, P, P, C.c_int, P, P, P, P]
        self._lib.sn_fetch.restype = None
        self._lib.sn_fetch.argtypes = [P, P]
        self._lib.sn_dump_compact.restype = C.c_int
        self._lib.sn_dump_compact.argtypes = [C.c_char_p]

    def run(self, p, src, fel, ad8, dxc=1.0, dyc=1.0, gt=(0.0, 1.0, 0.0, 1.0), cols=(), rows=(), ids=(), sw=False, p_nodata=P_NODATA, src_nodata=SRC_NODATA,
            dump=None):
        ny, nx = p.shape
        p = np.ascontiguousarray(p, np.int16)
        src = np.ascontiguousarray(src, np.int32)
        fel = np.ascontiguousarray(fel, np.float32)
        ad8 = np.ascontiguousarray(ad8, np.float32)
        dxc = np.ascontiguousarray(np.broadcast_to(np.asarray(dxc, np.float64), (ny,)))
        dyc = np.ascontiguousarray(np.broadcast_to(np.asarray(dyc, np.float64), (ny,)))
        gt = np.ascontiguousarray(gt, np.float64)
        cols, rows, ids = (np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1)) for a in (cols, rows, ids))
        ordg = np.empty((ny, nx), np.int16)
        w = np.empty((ny, nx), np.int32)
        nl, npt = C.c_int64(0), C.c_int64(0)
        rc = self._lib.sn_run(nx, ny, p.ctypes.data, p_nodata, src.ctypes.data, src_nodata, fel.ctypes.data, ad8.ctypes.data, dxc.ctypes.data, dyc.ctypes.data,
                              abs(float(dxc[ny // 2])), abs(float(dyc[ny // 2])), gt.ctypes.data, cols.size, cols.ctypes.data, rows.ctypes.data, ids.ctypes.data,
                              int(bool(sw)), ordg.ctypes.data, w.ctypes.data, C.addressof(nl), C.addressof(npt))
        if rc != 0:
            raise MemoryError("streamnet restatement failed")
        tree = np.empty((nl.value, 9), np.int64)
        coord = np.empty((npt.value, 5), np.float64)
        self._lib.sn_fetch(tree.ctypes.data, coord.ctypes.data)
        if dump is not None and self._lib.sn_dump_compact(str(dump).encode()) != 0:
            raise OSError(f"cannot write {dump}")
        return ordg, w, tree, coord


def compile(dirpath):
    lib = os.path.join(str(dirpath), "libstreamnet_restate.so")
    subprocess.run(["c++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-o", lib, SRC], check=True)
    return Restatement(lib)


# ---- inputs of the golden runs ----------------------------------------------------------------------------------------------------------
def geotransform(nx, ny, dx, dy, geographic):
    return (-111.9, dx, 0.0, 41.9, 0.0, -dy) if geographic else (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)


def inputs(name):
    """(case file, p, src int16): src = ad8 >= THRESH, nodata where ad8 is, a few cells raised to 2.  The cases' edge cells have no direction, so
    no stream of theirs leaves the raster: the stream end nearest to the west edge is led straight to it (p = 5, src = 1, the edge cell included)."""
    g = np.load(os.path.join(HERE, "golden", f"case_{name}.npz"))
    p, ad8 = g["p"].copy(), g["ad8"]
    stream = (ad8 >= THRESH[name]) & (p != P_NODATA)
    src = np.where(stream, 1, 0).astype(np.int16)
    src[ad8 < -0.5] = SRC_NODATA
    rng = np.random.default_rng(7300 + p.shape[0] + p.shape[1])
    twos = rng.choice(np.flatnonzero(stream), 3, replace=False)
    src.flat[twos] = 2                                                  # the terminal test is src != 1: a link ends above a 2
    _, recv, _ = stream_graph(p, src)
    nx = p.shape[1]
    ends = [int(c) for c in np.flatnonzero(stream) if recv[c] < 0 or not stream.flat[recv[c]]]
    e = min(ends, key=lambda c: c % nx)
    y, x = divmod(e, nx)
    p[y, :x + 1] = 5
    src[y, :x + 1] = 1
    return g, p, src


def stream_graph(p, src, p_nodata=P_NODATA, src_nodata=SRC_NODATA):
    """(stream mask, receiver's linear index or -1, number of stream cells draining into each cell)."""
    ny, nx = p.shape
    stream = (src != src_nodata) & (src > 0) & (p != p_nodata)
    recv = np.full(p.size, -1, np.int64)
    nin = np.zeros(p.size, np.int64)
    for c in np.flatnonzero(stream):
        y, x = divmod(int(c), nx)
        k = int(p[y, x])
        if 1 <= k <= 8 and 0 <= x + DX_[k] < nx and 0 <= y + DY_[k] < ny:
            r = (y + DY_[k]) * nx + x + DX_[k]
            recv[c] = r
            if stream.flat[r]:
                nin[r] += 1
    return stream, recv, nin


def outlets_for(p, src):
    """(cols, rows, ids): on a junction cell, mid-link, on a source cell, on an off-stream cell, off the raster, two on one cell."""
    ny, nx = p.shape
    stream, recv, nin = stream_graph(p, src)
    cells = np.flatnonzero(stream)
    junction = int(cells[np.flatnonzero(nin[cells] >= 2)[len(np.flatnonzero(nin[cells] >= 2)) // 2]])
    mids = [int(c) for c in cells if nin[c] == 1 and recv[c] >= 0 and stream.flat[recv[c]] and nin[recv[c]] == 1]
    mid = mids[len(mids) // 2]
    source = int(cells[np.flatnonzero(nin[cells] == 0)[3]])
    off = int(np.flatnonzero(~stream.ravel() & (p.ravel() > 0) & (src.ravel() == 0))[p.size // 7])
    twice = mids[len(mids) // 4]
    pick = [junction, mid, source, off, twice, twice]
    cols = [c % nx for c in pick] + [nx + 5]
    rows = [c // nx for c in pick] + [ny // 3]
    ids = [17, 3, 250, 42, 9001, 5, 64]
    return np.array(cols, np.int32), np.array(rows, np.int32), np.array(ids, np.int32)


# ---- hand-built rasters (at most 12 x 12) -------------------------------------------------------------------------------------------------
def _blank(ny=9, nx=10):
    p = np.full((ny, nx), 7, np.int16)            # everything drains south
    src = np.zeros((ny, nx), np.int16)
    return p, src


def small_rasters():
    """name -> (p, src): fel and ad8 are made by small_fields()."""
    out = {}
    p, s = _blank(); s[4, 5] = 1; out["one_cell"] = (p, s)
    p, s = _blank(); s[2:7, 4] = 1; out["straight"] = (p, s)
    p, s = _blank()
    for i in range(3):
        p[1 + i, 2 + i] = 8; s[1 + i, 2 + i] = 1; p[1 + i, 8 - i] = 6; s[1 + i, 8 - i] = 1
    s[4:8, 5] = 1; out["y"] = (p, s)
    p, s = _blank()
    p[3, 3] = 8; p[3, 5] = 6; p[4, 3] = 1; p[4, 5] = 5; s[3, 3] = s[3, 5] = s[4, 3] = s[4, 5] = 1
    p[2, 2] = 8; s[2, 2] = 1; p[4, 2] = 1; s[4, 2] = 1
    s[4:8, 4] = 1; out["fourway"] = (p, s)
    p, s = _blank()
    p[2, 3] = 8; p[2, 5] = 6; s[2, 3] = s[2, 5] = 1; s[3, 4] = 1; p[3, 3] = 8; s[3, 3] = 1; p[3, 5] = 6; s[3, 5] = 1; s[4:8, 4] = 1
    out["adjacent_junctions"] = (p, s)
    p, s = _blank(); s[2:7, 4] = 1; p[4, 4] = P_NODATA; out["stream_cell_without_p"] = (p, s)
    p, s = _blank()
    p[4, :] = 1; s[4, 6:] = 1; p[5, :] = 5; s[5, :4] = 1; p[:4, 2] = 3; s[:4, 2] = 1; s[6:, 7] = 1
    p[4, 2] = 3; out["off_each_edge"] = (p, s)
    p, s = _blank(); s[1:8, 4] = 1; s[3, 4] = SRC_NODATA; s[6, 4] = SRC_NODATA; s[2, 5] = SRC_NODATA; out["src_nodata_on_stream"] = (p, s)
    p, s = _blank(); out["no_stream"] = (p, s)
    p, s = _blank(); s[:] = 1; p[:, :5] = 8; p[:, 5:] = 6; p[8, :] = 1; p[0, 0] = P_NODATA; s[0, 0] = 0; out["all_stream"] = (p, s)
    return out


def small_fields(p):
    ny, nx = p.shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    fel = (100.0 - 1.5 * yy + 0.25 * np.abs(xx - nx // 2)).astype(np.float32)
    ad8 = (1.0 + yy * nx + xx).astype(np.float32)
    return fel, ad8


SMALL_GT = (200.0, 10.0, 0.0, 900.0, 0.0, -20.0)
SMALL_DX, SMALL_DY = 10.0, 20.0
SMALL_OUTLETS = (np.array([4, 4], np.int32), np.array([5, 2], np.int32), np.array([8, 12], np.int32))   # on column 4: most of the streams


def load_golden(name):
    g = np.load(os.path.join(HERE, "golden", f"streamnet_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def case_fields(name):
    """fel, ad8 and the per-row cell sizes of a committed case."""
    g = np.load(os.path.join(HERE, "golden", f"case_{name}.npz"))
    return {k: g[k] for k in ("fel", "ad8", "dxc", "dyc", "dx", "dy", "geographic")}


def assert_equals_golden(tag, got, g, variant, prefix=""):
    """got = (ord, w, tree rows, coord rows) against the reference's rasters and the bytes of its -tree / -coord files."""
    ordg, w, tree, coord = got
    k = lambda s: f"{prefix}{s}_{variant}"  # noqa: E731
    assert np.array_equal(ordg, g[k("ord")]), f"{tag}: {int(np.sum(ordg != g[k('ord')]))} order cells differ"
    assert np.array_equal(w, g[k("w")]), f"{tag}: {int(np.sum(w != g[k('w')]))} watershed cells differ"
    assert tree_text(tree).encode() == bytes(g[k("tree")]), f"{tag}: -tree differs"
    assert coord_text(coord).encode() == bytes(g[k("coord")]), f"{tag}: -coord differs"
