"""DinfDistDown's semantics as a plain C program (tests/distdown/distdown_restate.c): a literal Kahn queue over the whole raster.

    compile(dirpath)   builds the shared library with `cc` into dirpath (a pytest temporary directory) and returns a Restatement
    Restatement(ang, src, fel, stat, kind, weights, contcheck, dxc, dyc, ...)   the reference's raster, float32 (nodata -FLT_MAX)

tests/test_distdown_restatement.py holds it to every golden of tests/golden/distdown_*.npz bit for bit, so that the GPU tests can use
it at sizes the goldens do not cover.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "distdown", "distdown_restate.c")
STATS = {"ave": 0, "max": 1, "min": 2}
KINDS = {"h": 0, "v": 1, "p": 2, "s": 3}
ANG_NODATA = -3.402823466e38
FEL_NODATA = -3.0e38


class Restatement:
    def __init__(self, lib_path):
        self._lib = C.CDLL(lib_path)
        P = C.c_void_p
        self._lib.distdown.restype = C.c_int
        self._lib.distdown.argtypes = [C.c_int, C.c_int, P, C.c_float, P, C.c_float, P, P, C.c_float, P, P, C.c_int, C.c_int, C.c_int, P]

    def __call__(self, ang, src, fel=None, stat="ave", kind="v", weights=None, contcheck=True, dxc=1.0, dyc=1.0, ang_nodata=ANG_NODATA,
                 fel_nodata=FEL_NODATA, weights_nodata=-9999.0):
        ny, nx = ang.shape
        ang = np.ascontiguousarray(ang, np.float32)
        src = np.ascontiguousarray(src, np.int16)
        fel = None if fel is None else np.ascontiguousarray(fel, np.float32)
        weights = None if weights is None else np.ascontiguousarray(weights, np.float32)
        dxc = np.ascontiguousarray(np.broadcast_to(np.asarray(dxc, np.float64), (ny,)))
        dyc = np.ascontiguousarray(np.broadcast_to(np.asarray(dyc, np.float64), (ny,)))
        if kind != "h" and fel is None:
            raise ValueError("fel is needed for kinds v, p and s")
        out = np.empty((ny, nx), np.float32)
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        rc = self._lib.distdown(nx, ny, ptr(ang), float(ang_nodata), ptr(fel), float(fel_nodata), ptr(src), ptr(weights), float(weights_nodata),
                                ptr(dxc), ptr(dyc), STATS[stat], KINDS[kind], int(bool(contcheck)), ptr(out))
        if rc != 0:
            raise MemoryError("distdown restatement: out of memory")
        return out


def compile(dirpath):
    lib = os.path.join(str(dirpath), "libdistdown_restate.so")
    subprocess.run(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-o", lib, SRC, "-lm"], check=True)
    return Restatement(lib)


def load_golden(name):
    g = np.load(os.path.join(HERE, "golden", f"distdown_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def golden_names():
    return sorted(f[len("distdown_"):-len(".npz")] for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("distdown_") and f.endswith(".npz"))


def variants():
    """(stat, kind, suffix) of every golden raster: suffix '' default, '_nc' without the contamination check, '_wg' with weights."""
    return [(s, k, v) for s in STATS for k in KINDS for v in ("", "_nc", "_wg")]
