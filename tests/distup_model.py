"""DinfDistUp's semantics as a plain C program (tests/distup/distup_restate.c): a literal Kahn queue over the whole raster.

    compile(dirpath)   builds the shared library with `cc` into dirpath (a pytest temporary directory) and returns a Restatement
    Restatement(ang, fel, stat, kind, weights, contcheck, thresh, dxc, dyc, ...)   the reference's raster, float32 (nodata -FLT_MAX)

tests/test_distup_restatement.py holds it to every golden of tests/golden/distup_*.npz bit for bit, so that the GPU tests can use it at
sizes the goldens do not cover.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "distup", "distup_restate.c")
STATS = {"ave": 0, "max": 1, "min": 2}
KINDS = {"h": 0, "v": 1, "p": 2, "s": 3}
ANG_NODATA = -3.402823466e38
FEL_NODATA = -3.0e38
THRESH_RUNS = (("ave", "h"), ("max", "v"))   # the -thresh goldens (du_<stat>_<kind>_t), threshold THRESH
V_WG_RUNS = ("ave",)   # v ignores -wg (the reference comments the weight code out): one v -wg golden shows it, the others would repeat v
THRESH = 0.3


class Restatement:
    def __init__(self, lib_path):
        self._lib = C.CDLL(lib_path)
        P = C.c_void_p
        self._lib.distup.restype = C.c_int
        self._lib.distup.argtypes = [C.c_int, C.c_int, P, C.c_float, P, C.c_float, P, C.c_float, P, P, C.c_int, C.c_int, C.c_int, C.c_float, P]

    def __call__(self, ang, fel=None, stat="ave", kind="h", weights=None, contcheck=True, thresh=0.0, dxc=1.0, dyc=1.0, ang_nodata=ANG_NODATA,
                 fel_nodata=FEL_NODATA, weights_nodata=-9999.0):
        ny, nx = ang.shape
        ang = np.ascontiguousarray(ang, np.float32)
        fel = None if fel is None else np.ascontiguousarray(fel, np.float32)
        weights = None if weights is None else np.ascontiguousarray(weights, np.float32)
        dxc = np.ascontiguousarray(np.broadcast_to(np.asarray(dxc, np.float64), (ny,)))
        dyc = np.ascontiguousarray(np.broadcast_to(np.asarray(dyc, np.float64), (ny,)))
        if kind != "h" and fel is None:
            raise ValueError("fel is needed for kinds v, p and s")
        out = np.empty((ny, nx), np.float32)
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        rc = self._lib.distup(nx, ny, ptr(ang), float(ang_nodata), ptr(fel), float(fel_nodata), ptr(weights), float(weights_nodata), ptr(dxc), ptr(dyc),
                              STATS[stat], KINDS[kind], int(bool(contcheck)), float(thresh), ptr(out))
        if rc != 0:
            raise MemoryError("distup restatement: out of memory")
        return out


def compile(dirpath):
    lib = os.path.join(str(dirpath), "libdistup_restate.so")
    subprocess.run(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-o", lib, SRC, "-lm"], check=True)
    return Restatement(lib)


def load_golden(name):
    g = np.load(os.path.join(HERE, "golden", f"distup_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def golden_names():
    return sorted(f[len("distup_"):-len(".npz")] for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("distup_") and f.endswith(".npz"))


def variants():
    """(stat, kind, suffix) of every golden raster: suffix '' default, '_nc' without the contamination check, '_wg' with weights (for v only
    V_WG_RUNS), '_t' with -thresh THRESH (THRESH_RUNS)."""
    return ([(s, k, v) for s in STATS for k in KINDS for v in ("", "_nc", "_wg") if not (k == "v" and v == "_wg" and s not in V_WG_RUNS)]
            + [(s, k, "_t") for s, k in THRESH_RUNS])


def run(restate, g, stat, kind, sfx):
    """The restatement on golden g in the configuration of variant suffix sfx."""
    return restate(g["ang"], g["fel"], stat=stat, kind=kind, weights=g["wg"] if sfx == "_wg" else None, contcheck=sfx != "_nc",
                   thresh=THRESH if sfx == "_t" else 0.0, dxc=g["dxc"], dyc=g["dyc"])
