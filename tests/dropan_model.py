"""DropAnalysis' semantics as a serial C++ program (tests/dropan/dropan_restate.cpp): the FIFO queue of the reference on one rank, float sums in
the order the queue pops the cells, the ladder and the table writer.

    compile(dirpath)              builds the shared library with g++ into dirpath (a pytest temporary directory) and returns a Restatement
    Restatement.ladder(...)       the thresholds, float32
    Restatement.threshold(...)    one threshold: float sums, counts, length, the order / elevOut grids and the two drop lists
    Restatement.run(...)          all thresholds + total area + table: what the tool does
    Restatement.table(...)        the table file and the console lines from float sums

tests/test_dropan_restatement.py holds it to every 1-rank golden of tests/golden/dropan_*.npz byte for byte, so that the GPU tests can use it at
sizes the goldens do not cover.  The exact-sum helpers of the GPU tests live here too.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "dropan", "dropan_restate.cpp")
GOLDEN = os.path.join(HERE, "golden")
CASES = ("fourway_mask", "geographic", "holes", "plain", "rect_dxdy")
P_NODATA = -32768
SSA_NODATA = -1.0
ORDER_NODATA = -32768
ELEV_NODATA = np.float32(-3.402823466e38)
U = 2.0 ** -53     # unit roundoff of fp64


def _f64(a, n):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), (n,)))


def gamma(n):
    """gamma_n = n u / (1 - n u): the bound of n roundings (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)."""
    return n * U / (1.0 - n * U)


def text_of(a):
    """bytes of a text stored in an npz as a uint8 array"""
    return np.asarray(a, np.uint8).tobytes()


def load_golden(name):
    g = dict(np.load(os.path.join(GOLDEN, f"case_{name}.npz")))
    g.update(np.load(os.path.join(GOLDEN, f"dropan_{name}.npz")))
    return g


def parse_table(text):
    """(rows [n][9] float64, optimum) of a table file"""
    lines = text.decode().strip().split("\n")
    assert lines[0].startswith("Threshold, DrainDen") and lines[-1].startswith("Optimum Threshold Value: ")
    rows = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:-1]], np.float64).reshape(-1, 9)
    return rows, float(lines[-1].split(":")[1])


def console_t(console):
    """the Tval entries of the console lines that have one"""
    lines = console.decode().split("\n")
    first = next(i for i, ln in enumerate(lines) if ln.startswith("Threshold DrainDen"))
    ts = []
    for ln in lines[first + 1:]:
        if "Value for optimum" in ln:
            break
        last = ln.replace(" - ", " x ").split()[-1]
        if last != "x":
            ts.append(float(last))
    return np.array(ts)


def sums_from_drops(d1, d2):
    """s1, s1sq, s2, s2sq: the correctly rounded sums of the drops and of their float squares (math.fsum), as float64"""
    sq = lambda d: (d * d).astype(np.float32)  # noqa: E731  (the float square, as the reference forms it)
    return [math.fsum(d1.astype(np.float64)), math.fsum(sq(d1).astype(np.float64)), math.fsum(d2.astype(np.float64)), math.fsum(sq(d2).astype(np.float64))]


def abs_sums_from_drops(d1, d2):
    sq = lambda d: (d * d).astype(np.float32)  # noqa: E731
    return [math.fsum(np.abs(d1).astype(np.float64)), math.fsum(sq(d1).astype(np.float64)), math.fsum(np.abs(d2).astype(np.float64)), math.fsum(sq(d2).astype(np.float64))]


def exact_length(order, p, dxc, dyc, p_nodata=P_NODATA):
    """(math.fsum of the link lengths, number of links): every cell with a record that points at a cell with a record is one link, measured with
    the cell sizes of the RECEIVING cell's row"""
    ny, nx = order.shape
    dx = (0, 1, 1, 0, -1, -1, -1, 0, 1)
    dy = (0, 0, -1, -1, -1, 0, 1, 1, 1)
    terms = []
    has = order != ORDER_NODATA
    for k in range(1, 9):
        ys, xs = np.nonzero(has & (p == k))
        yr, xr = ys + dy[k], xs + dx[k]
        ok = (xr >= 0) & (xr < nx) & (yr >= 0) & (yr < ny)
        yr, xr = yr[ok], xr[ok]
        yr = yr[has[yr, xr]]
        if k in (1, 5):
            terms.append(dxc[yr])
        elif k in (3, 7):
            terms.append(dyc[yr])
        else:
            terms.append(np.sqrt(dxc[yr] * dxc[yr] + dyc[yr] * dyc[yr]))
    t = np.concatenate(terms) if terms else np.zeros(0)
    return math.fsum(t), int(t.size)


class Restatement:
    def __init__(self, lib_path):
        self._lib = C.CDLL(lib_path)
        P, I, F, D = C.c_void_p, C.c_int, C.c_float, C.c_double
        self._lib.da_ladder.restype = None
        self._lib.da_ladder.argtypes = [F, F, I, I, P]
        self._lib.da_threshold.restype = None
        self._lib.da_threshold.argtypes = [I, I, P, C.c_int16, P, P, F, P, P, F, P, P, P, P, P, P, P]
        self._lib.da_total_area.restype = I
        self._lib.da_total_area.argtypes = [I, I, P, P, C.c_int16, P, F, P, P, I, D, D, P]
        self._lib.da_table.restype = I
        self._lib.da_table.argtypes = [I, P, P, P, P, P, P, P, P, F, P, I, P, I, P, P]

    def ladder(self, tmin, tmax, nthresh, steptype):
        out = np.zeros(nthresh, np.float32)
        self._lib.da_ladder(float(tmin), float(tmax), int(nthresh), int(steptype), out.ctypes.data)
        return out

    def threshold(self, p, fel, ssa, dxc, dyc, thresh, p_nodata=P_NODATA, ssa_nodata=SSA_NODATA):
        """dict: s (float32[4]), n1, n2, length, order, elev, drops1, drops2"""
        ny, nx = p.shape
        p, fel, ssa = np.ascontiguousarray(p, np.int16), np.ascontiguousarray(fel, np.float32), np.ascontiguousarray(ssa, np.float32)
        dxc, dyc = _f64(dxc, ny), _f64(dyc, ny)
        s, n, length = np.zeros(4, np.float32), np.zeros(2, np.int64), np.zeros(1, np.float64)
        order, elev = np.zeros((ny, nx), np.int16), np.zeros((ny, nx), np.float32)
        d1, d2 = np.zeros(ny * nx, np.float32), np.zeros(ny * nx, np.float32)
        self._lib.da_threshold(nx, ny, p.ctypes.data, int(p_nodata), fel.ctypes.data, ssa.ctypes.data, float(ssa_nodata), dxc.ctypes.data, dyc.ctypes.data,
                               float(np.float32(thresh)), s.ctypes.data, n.ctypes.data, length.ctypes.data, order.ctypes.data, elev.ctypes.data, d1.ctypes.data, d2.ctypes.data)
        return {"s": s, "n1": int(n[0]), "n2": int(n[1]), "length": float(length[0]), "order": order, "elev": elev, "drops1": d1[:n[0]].copy(), "drops2": d2[:n[1]].copy()}

    def total_area(self, ad8, p, ssa, cols, rows, dxA, dyA, p_nodata=P_NODATA, ssa_nodata=SSA_NODATA):
        """float32, or None when an outlet lies on a cell without a direction"""
        ny, nx = p.shape
        ad8, ssa = np.ascontiguousarray(ad8, np.float32), np.ascontiguousarray(ssa, np.float32)
        p, cols, rows = np.ascontiguousarray(p, np.int16), np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(rows, np.int32)
        out = np.zeros(1, np.float32)
        rc = self._lib.da_total_area(nx, ny, ad8.ctypes.data, p.ctypes.data, int(p_nodata), ssa.ctypes.data, float(ssa_nodata), cols.ctypes.data, rows.ctypes.data,
                                     int(cols.size), float(dxA), float(dyA), out.ctypes.data)
        return None if rc else out[0]

    def table(self, thresh, n1, n2, s, length, total_area):
        """(table bytes, console bytes, optimum or None); s: float32 [nthresh][4]"""
        nt = len(thresh)
        thresh = np.ascontiguousarray(thresh, np.float32)
        n1, n2 = np.ascontiguousarray(n1, np.int64), np.ascontiguousarray(n2, np.int64)
        cols = [np.ascontiguousarray(np.asarray(s, np.float32).reshape(nt, 4)[:, k]) for k in range(4)]
        length = np.ascontiguousarray(length, np.float64)
        tab, con = C.create_string_buffer(256 * nt + 512), C.create_string_buffer(256 * nt + 1024)
        opt, found = C.c_float(0), C.c_int(0)
        rc = self._lib.da_table(nt, thresh.ctypes.data, n1.ctypes.data, n2.ctypes.data, cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data, cols[3].ctypes.data,
                                length.ctypes.data, float(total_area), C.cast(tab, C.c_void_p), len(tab), C.cast(con, C.c_void_p), len(con), C.addressof(opt),
                                C.addressof(found))
        assert rc >= 0
        return tab.value, con.value, (np.float32(opt.value) if found.value else None)

    def run(self, ad8, p, fel, ssa, cols, rows, dxc, dyc, tmin=5.0, tmax=500.0, nthresh=10, steptype=0, p_nodata=P_NODATA, ssa_nodata=SSA_NODATA):
        """dict: thresh, per (list of threshold() dicts), total_area, table, console, optimum"""
        ny, nx = p.shape
        dxc, dyc = _f64(dxc, ny), _f64(dyc, ny)
        thresh = self.ladder(tmin, tmax, nthresh, steptype)
        per = [self.threshold(p, fel, ssa, dxc, dyc, t, p_nodata, ssa_nodata) for t in thresh]
        area = self.total_area(ad8, p, ssa, cols, rows, abs(dxc[ny // 2]), abs(dyc[ny // 2]), p_nodata, ssa_nodata)
        tab, con, opt = self.table(thresh, [q["n1"] for q in per], [q["n2"] for q in per], np.array([q["s"] for q in per]), [q["length"] for q in per], area)
        return {"thresh": thresh, "per": per, "total_area": area, "table": tab, "console": con, "optimum": opt}


def compile(dirpath):
    lib = os.path.join(str(dirpath), "dropan_restate.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", lib], check=True)
    return Restatement(lib)
