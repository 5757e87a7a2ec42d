"""RetLimFlow's and DinfAvalanche's semantics as a plain C program (tests/aval/aval_restate.c): a literal Kahn queue over the whole raster.

    compile(dirpath)                     builds the shared library with `cc` into dirpath (a pytest temporary directory); returns a Restatement
    Restatement.retlimflow(ang, wg, rc, ...)             qrl, float32 (nodata -FLT_MAX)
    Restatement.dinfavalanche(ang, fel, ass, ...)        (rz, dfs, taint): float32, float32, bool

`taint` marks the cells where one of the reference's decisions is so close that a runout angle off by TOL_ULPS float ulps could flip it
and change the cell's record, and everything that takes from such a cell: those cells are left out when a GPU result is compared.  The
tolerance is derived, not measured: the host atanf of glibc is documented at 1 ulp, the device evaluates atan in double and rounds once
(0.5 ulp), and the scaling by 180 / PI with the final rounding adds at most 1 ulp.

tests/test_aval_restatement.py holds the restatement to every golden of tests/golden/aval_*.npz, so that the GPU tests can use it at
sizes the goldens do not cover.
"""
import ctypes as C
import os
import platform
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "aval", "aval_restate.c")
ANG_NODATA = -3.402823466e38
FEL_NODATA = -3.0e38
WG_NODATA = -9999.0
RC_NODATA = -9999.0
ASS_NODATA = -32768
TOL_ULPS = 3                      # rz on untainted cells: GPU vs reference
MAX_TAINT_SHARE = 0.01            # of the cells with rz data, per run
DEFAULT = (0.2, 18.0)             # (thresh, alpha) of src/DinfAvalanchemn.cpp:55
OTHER = (0.35, 25.0)              # the second golden configuration


def libc_tag():
    return "-".join(platform.libc_ver())


def default_geo(ny, dxc, dyc):
    """{xleftedge, ytopedge, dlon, dlat} the library assumes when -direct gets no geotransform."""
    dlon, dlat = float(np.atleast_1d(dxc)[0]), float(np.atleast_1d(dyc)[0])
    return (0.0, ny * dlat, dlon, dlat)


class Restatement:
    def __init__(self, lib_path):
        self._lib = C.CDLL(lib_path)
        P = C.c_void_p
        self._lib.retlimflow.restype = C.c_int
        self._lib.retlimflow.argtypes = [C.c_int, C.c_int, P, C.c_float, P, C.c_float, P, C.c_float, P, P, P]
        self._lib.dinfavalanche.restype = C.c_int
        self._lib.dinfavalanche.argtypes = [C.c_int, C.c_int, P, C.c_float, P, C.c_float, P, C.c_int16, P, P, C.c_float, C.c_float, C.c_int, P, C.c_int, C.c_int,
                                            P, P, P]

    @staticmethod
    def _cells(ny, dxc, dyc):
        return (np.ascontiguousarray(np.broadcast_to(np.asarray(dxc, np.float64), (ny,))), np.ascontiguousarray(np.broadcast_to(np.asarray(dyc, np.float64), (ny,))))

    def retlimflow(self, ang, wg, rc, dxc=1.0, dyc=1.0, ang_nodata=ANG_NODATA, wg_nodata=WG_NODATA, rc_nodata=RC_NODATA):
        ny, nx = ang.shape
        ang, wg, rc = (np.ascontiguousarray(a, np.float32) for a in (ang, wg, rc))
        dxc, dyc = self._cells(ny, dxc, dyc)
        out = np.empty((ny, nx), np.float32)
        if self._lib.retlimflow(nx, ny, ang.ctypes.data, float(ang_nodata), wg.ctypes.data, float(wg_nodata), rc.ctypes.data, float(rc_nodata), dxc.ctypes.data,
                                dyc.ctypes.data, out.ctypes.data) != 0:
            raise MemoryError("retlimflow restatement: out of memory")
        return out

    def dinfavalanche(self, ang, fel, ass, thresh=DEFAULT[0], alpha=DEFAULT[1], direct=False, dxc=1.0, dyc=1.0, geo=None, geographic=False, ang_nodata=ANG_NODATA,
                      fel_nodata=FEL_NODATA, ass_nodata=ASS_NODATA, tol=TOL_ULPS):
        ny, nx = ang.shape
        ang, fel = (np.ascontiguousarray(a, np.float32) for a in (ang, fel))
        ass = np.ascontiguousarray(ass, np.int16)
        dxc, dyc = self._cells(ny, dxc, dyc)
        geo = np.asarray(default_geo(ny, dxc, dyc) if geo is None else geo, np.float64)
        rz = np.empty((ny, nx), np.float32)
        dfs = np.empty((ny, nx), np.float32)
        taint = np.empty((ny, nx), np.uint8)
        if self._lib.dinfavalanche(nx, ny, ang.ctypes.data, float(ang_nodata), fel.ctypes.data, float(fel_nodata), ass.ctypes.data, int(ass_nodata), dxc.ctypes.data,
                                   dyc.ctypes.data, float(thresh), float(alpha), 0 if direct else 1, geo.ctypes.data, int(bool(geographic)), int(tol),
                                   rz.ctypes.data, dfs.ctypes.data, taint.ctypes.data) != 0:
            raise MemoryError("dinfavalanche restatement: out of memory")
        return rz, dfs, taint.astype(bool)


def compile(dirpath):
    lib = os.path.join(str(dirpath), "libaval_restate.so")
    subprocess.run(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-o", lib, SRC, "-lm"], check=True)
    return Restatement(lib)


def load_golden(name):
    g = np.load(os.path.join(HERE, "golden", f"aval_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def golden_names():
    return sorted(f[len("aval_"):-len(".npz")] for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("aval_") and f.endswith(".npz"))


def variants():
    """(suffix, direct, (thresh, alpha)) of every avalanche golden pair rz<suffix> / dfs<suffix>."""
    return [("_path", False, DEFAULT), ("_direct", True, DEFAULT), ("_path_o", False, OTHER), ("_direct_o", True, OTHER)]


def golden_geo(g):
    return tuple(float(v) for v in g["geo"]), bool(g["geographic"])


def run_aval(restate, g, direct, ta):
    geo, geographic = golden_geo(g)
    return restate.dinfavalanche(g["ang"], g["fel"], g["ass"], thresh=ta[0], alpha=ta[1], direct=direct, dxc=g["dxc"], dyc=g["dyc"], geo=geo, geographic=geographic)


def ulps(a, b):
    """Distance of two float32 arrays in ulps (int64)."""
    def order(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(2 ** 31) - i, i)
    return np.abs(order(a) - order(b))


def compare_aval(rz, dfs, ref_rz, ref_dfs, taint, what=""):
    """The GPU rule: on untainted cells the same cells have data, dfs is bit-equal and rz is within TOL_ULPS; tainted cells are at most
    MAX_TAINT_SHARE of the cells with rz data.  Returns a list of complaints (empty: fine)."""
    bad = []
    has = ref_rz > -1e30
    share = float(taint.sum()) / max(int(has.sum()), 1)
    if share > MAX_TAINT_SHARE:
        bad.append(f"{what}: {int(taint.sum())} tainted cells = {share:.4f} of the {int(has.sum())} cells with rz data (limit {MAX_TAINT_SHARE})")
    ok = ~taint
    if not np.array_equal((rz > -1e30) & ok, has & ok):
        bad.append(f"{what}: the set of cells with rz data differs on {int(np.sum(((rz > -1e30) != has) & ok))} untainted cells")
    if not np.array_equal(dfs.view(np.uint32)[ok], ref_dfs.view(np.uint32)[ok]):
        d = (dfs.view(np.uint32) != ref_dfs.view(np.uint32)) & ok
        j, i = np.argwhere(d)[0]
        bad.append(f"{what}: dfs differs on {int(d.sum())} untainted cells, first ({j}, {i}): {dfs[j, i]!r} vs {ref_dfs[j, i]!r}")
    both = ok & has & (rz > -1e30)
    u = ulps(rz, ref_rz)
    worst = int(u[both].max()) if both.any() else 0
    print(f"{what}: cells with rz {int(has.sum())}, tainted {int(taint.sum())} ({share:.5f}), worst rz distance on untainted cells {worst} ulps")
    if worst > TOL_ULPS:
        j, i = np.argwhere(both & (u > TOL_ULPS))[0]
        bad.append(f"{what}: rz is {worst} ulps off (limit {TOL_ULPS}), first ({j}, {i}): {rz[j, i]!r} vs {ref_rz[j, i]!r}")
    return bad
