"""FlowDirCond's, D8VDistToStrm's and SlopeAveDown's semantics as a plain C program (tests/d8last/d8last_restate.c): literal Kahn queues over
the whole raster; SlopeAveDown as niter full queue passes that update ed / dd in place, as the reference does.

    compile(dirpath)   builds the shared library with `cc` into dirpath (a pytest temporary directory) and returns a Restatement
    Restatement.flowdircond(p, z, z_nodata)                      the conditioned elevations, float32
    Restatement.vdist(p, fel, src, thresh)                        the vertical distance raster, float32 (nodata -FLT_MAX)
    Restatement.slopeavedown(p, fel, dn, dxc, dyc, fel_nodata)    the slope raster, float32 (nodata -FLT_MAX)

tests/test_d8last_restatement.py holds it to every golden of tests/golden/d8last_*.npz bit for bit, so that the GPU tests can use it at
sizes the goldens do not cover.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "d8last", "d8last_restate.c")
P_NODATA = -32768
FEL_NODATA = -3.0e38
SRC_NODATA = -32768          # the Threshold raster's nodata, read as a LONG (tests/golden/make_golden_d8rev.py)
THRESH_AD8 = 40              # -thresh of the run with the contributing-area raster as -src
DN_FACTORS = (0.5, 2.5, 6.2)  # dn as multiples of the smaller cell size of the middle row: niter 1, 3 and 7


def niter_of(dn, dxc, dyc):
    """int(dn / min(dxA, dyA)) + 1 with the cell sizes of the middle row (src/SlopeAveDown.cpp:172, src/tiffIO.cpp:155-156)."""
    dxc, dyc = np.atleast_1d(np.asarray(dxc, np.float64)), np.atleast_1d(np.asarray(dyc, np.float64))
    return int(float(dn) / min(abs(float(dxc[dxc.size // 2])), abs(float(dyc[dyc.size // 2]))) + 1.0)


def dns_of(dxc, dyc):
    """The three -dn values of the goldens for a raster with these per-row cell sizes."""
    dxc, dyc = np.atleast_1d(np.asarray(dxc, np.float64)), np.atleast_1d(np.asarray(dyc, np.float64))
    m = min(abs(float(dxc[dxc.size // 2])), abs(float(dyc[dyc.size // 2])))
    return tuple(round(f * m, 3) for f in DN_FACTORS)


class Restatement:
    def __init__(self, lib_path):
        self._lib = C.CDLL(lib_path)
        P = C.c_void_p
        self._lib.flowdircond.restype = C.c_int
        self._lib.flowdircond.argtypes = [C.c_int, C.c_int, P, C.c_int16, P, C.c_float, P]
        self._lib.d8vdist.restype = C.c_int
        self._lib.d8vdist.argtypes = [C.c_int, C.c_int, P, C.c_int16, P, P, C.c_int32, C.c_int32, P]
        self._lib.slopeavedown.restype = C.c_int
        self._lib.slopeavedown.argtypes = [C.c_int, C.c_int, P, C.c_int16, P, C.c_float, P, P, C.c_double, C.c_long, P]

    def flowdircond(self, p, z, z_nodata=FEL_NODATA, p_nodata=P_NODATA):
        ny, nx = p.shape
        p = np.ascontiguousarray(p, np.int16)
        z = np.ascontiguousarray(z, np.float32)
        out = np.empty((ny, nx), np.float32)
        if self._lib.flowdircond(nx, ny, p.ctypes.data, p_nodata, z.ctypes.data, float(z_nodata), out.ctypes.data) != 0:
            raise MemoryError("flowdircond restatement: out of memory")
        return out

    def vdist(self, p, fel, src, thresh=1, p_nodata=P_NODATA, src_nodata=SRC_NODATA):
        ny, nx = p.shape
        p = np.ascontiguousarray(p, np.int16)
        fel = np.ascontiguousarray(fel, np.float32)
        src = np.ascontiguousarray(src, np.int32)
        out = np.empty((ny, nx), np.float32)
        if self._lib.d8vdist(nx, ny, p.ctypes.data, p_nodata, fel.ctypes.data, src.ctypes.data, src_nodata, int(thresh), out.ctypes.data) != 0:
            raise MemoryError("d8vdist restatement: out of memory")
        return out

    def slopeavedown(self, p, fel, dn, dxc=1.0, dyc=1.0, fel_nodata=FEL_NODATA, p_nodata=P_NODATA, niter=None):
        ny, nx = p.shape
        p = np.ascontiguousarray(p, np.int16)
        fel = np.ascontiguousarray(fel, np.float32)
        dxc = np.ascontiguousarray(np.broadcast_to(np.asarray(dxc, np.float64), (ny,)))
        dyc = np.ascontiguousarray(np.broadcast_to(np.asarray(dyc, np.float64), (ny,)))
        if niter is None:
            niter = niter_of(dn, dxc, dyc)
        out = np.empty((ny, nx), np.float32)
        if self._lib.slopeavedown(nx, ny, p.ctypes.data, p_nodata, fel.ctypes.data, float(fel_nodata), dxc.ctypes.data, dyc.ctypes.data, float(dn), int(niter),
                                  out.ctypes.data) != 0:
            raise MemoryError("slopeavedown restatement: out of memory")
        return out


def compile(dirpath):
    lib = os.path.join(str(dirpath), "libd8last_restate.so")
    subprocess.run(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-o", lib, SRC, "-lm"], check=True)
    return Restatement(lib)


def load_golden(name):
    g = np.load(os.path.join(HERE, "golden", f"d8last_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def golden_names():
    return sorted(f[len("d8last_"):-len(".npz")] for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("d8last_") and f.endswith(".npz"))
