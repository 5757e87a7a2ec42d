"""D8HDistToStrm's and GageWatershed's semantics as a plain C program (tests/d8rev/d8rev_restate.c): a literal Kahn queue over the whole
raster, from the sources upstream.

    compile(dirpath)   builds the shared library with `cc` into dirpath (a pytest temporary directory) and returns a Restatement
    Restatement.dist(p, src, thresh, dxc, dyc)      the reference's distance raster, float32 (nodata -FLT_MAX)
    Restatement.gage(p, cols, rows, ids)            (gw int32 (nodata -2147483647), the -id file's text)

tests/test_d8rev_restatement.py holds it to every golden of tests/golden/d8rev_*.npz bit for bit and byte for byte, so that the GPU tests
can use it at sizes the goldens do not cover.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "d8rev", "d8rev_restate.c")
P_NODATA = -32768
SRC_NODATA = -32768          # the Threshold raster's nodata, read as a LONG (tests/golden/make_golden_d8rev.py)
GW_NODATA = -2147483647
THRESH_AD8 = 40              # -thresh of the run with the contributing-area raster as -src


def id_text(ids, towrite, dsids):
    """The -id file (src/gagewatershed.cpp:327-341)."""
    return "id iddown\n" + "".join(f"{int(i)} {int(d)}\n" for i, w, d in zip(ids, towrite, dsids) if w > 0)


def table_text(table):
    """Context.gagewatershed's (k, 2) id table as the -id file's text."""
    return "id iddown\n" + "".join(f"{int(i)} {int(d)}\n" for i, d in np.asarray(table).reshape(-1, 2))


class Restatement:
    def __init__(self, lib_path):
        self._lib = C.CDLL(lib_path)
        P = C.c_void_p
        self._lib.d8hdist.restype = C.c_int
        self._lib.d8hdist.argtypes = [C.c_int, C.c_int, P, C.c_int16, P, C.c_int32, C.c_int32, P, P, P]
        self._lib.gagews.restype = C.c_int
        self._lib.gagews.argtypes = [C.c_int, C.c_int, P, C.c_int16, C.c_int, P, P, P, P, P, P]

    def dist(self, p, src, thresh=1, dxc=1.0, dyc=1.0, p_nodata=P_NODATA, src_nodata=SRC_NODATA):
        ny, nx = p.shape
        p = np.ascontiguousarray(p, np.int16)
        src = np.ascontiguousarray(src, np.int32)
        dxc = np.ascontiguousarray(np.broadcast_to(np.asarray(dxc, np.float64), (ny,)))
        dyc = np.ascontiguousarray(np.broadcast_to(np.asarray(dyc, np.float64), (ny,)))
        out = np.empty((ny, nx), np.float32)
        rc = self._lib.d8hdist(nx, ny, p.ctypes.data, p_nodata, src.ctypes.data, src_nodata, int(thresh), dxc.ctypes.data, dyc.ctypes.data, out.ctypes.data)
        if rc != 0:
            raise MemoryError("d8hdist restatement: out of memory")
        return out

    def gage(self, p, cols, rows, ids, p_nodata=P_NODATA):
        ny, nx = p.shape
        p = np.ascontiguousarray(p, np.int16)
        cols, rows, ids = (np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1)) for a in (cols, rows, ids))
        n = cols.size
        gw = np.empty((ny, nx), np.int32)
        towrite = np.zeros(n + 1, np.int32)
        dsids = np.zeros(n + 1, np.int32)
        rc = self._lib.gagews(nx, ny, p.ctypes.data, p_nodata, n, cols.ctypes.data, rows.ctypes.data, ids.ctypes.data, gw.ctypes.data, towrite.ctypes.data,
                              dsids.ctypes.data)
        if rc != 0:
            raise MemoryError("gagews restatement: out of memory")
        return gw, id_text(ids, towrite[:n], dsids[:n])


def compile(dirpath):
    lib = os.path.join(str(dirpath), "libd8rev_restate.so")
    subprocess.run(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-o", lib, SRC, "-lm"], check=True)
    return Restatement(lib)


def load_golden(name):
    g = np.load(os.path.join(HERE, "golden", f"d8rev_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def golden_names():
    return sorted(f[len("d8rev_"):-len(".npz")] for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("d8rev_") and f.endswith(".npz"))
