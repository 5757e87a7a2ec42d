"""MoveOutletsToStrm's and ConnectDown's semantics as a plain C program (tests/outlets/outlets_restate.c): whole-raster loops, one rank.

    compile(dirpath)                          builds the shared library with `cc` into dirpath and returns a Restatement
    Restatement.moveoutlets(p, src, cols, rows, maxdist)   -> (columns, rows, dist_moved)
    Restatement.connectdown(p, w, ad8, movedist)           -> (ids, columns, rows, ad8max, moved columns, moved rows, id_down)
    Restatement.moveoutlets_strips / connectdown_strips    the same through a CPU model of the hand-over between row strips cut at `cuts`
    inputs(case) / outlet_points(...)         the inputs of the golden runs (shared with tests/golden/make_golden_outlets.py)
    small_rasters() / small_outlets(...)      the hand-built rasters
    move_record(...) / connect_records(...)   the text the recording OGR stand-in leaves for such results (tests/outlets/ogr_record_stub.h)

tests/test_outlets_restatement.py holds it to every golden of tests/golden/outlets_*.npz, so that the GPU tests can use it at sizes the goldens do
not cover.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import streamnet_model as SM

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "outlets", "outlets_restate.c")
P_NODATA = -32768
SRC_NODATA = -32768
W_NODATA = -2147483647
AD8_NODATA = -1.0
MAX_ID = 134217727            # TDX_CONNECTDOWN_MAX_ID of include/taudem_amd_outlets.h
CASES = SM.CASES
MAXDISTS = (50, 3)            # -md of the golden runs
MOVEDISTS = (10, 2)           # -d of the golden runs
DX_ = SM.DX_
DY_ = SM.DY_
SMALL_GT = (200.0, 10.0, 0.0, 900.0, 0.0, -20.0)


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1)).copy()


class Restatement:
    def __init__(self, lib_path):
        L = self._lib = C.CDLL(lib_path)
        P, I, LG = C.c_void_p, C.c_int, C.c_long
        L.or_moveoutlets.restype = I
        L.or_moveoutlets.argtypes = [I, I, P, C.c_int16, P, C.c_int32, I, LG, P, P, P]
        L.or_moveoutlets_step.restype = LG
        L.or_moveoutlets_step.argtypes = [I, I, P, C.c_int16, P, C.c_int32, I, I, I, LG, P, P, P, P]
        L.or_argmax_rows.restype = LG
        L.or_argmax_rows.argtypes = [I, I, I, P, C.c_int32, P, LG, P, P, P, P]
        L.or_id_range.restype = None
        L.or_id_range.argtypes = [I, I, P, C.c_int32, P, P]
        L.or_walkdown_round.restype = LG
        L.or_walkdown_round.argtypes = [I, I, P, P, I, I, I, LG, P, P, P, P]
        L.or_connectdown.restype = LG
        L.or_connectdown.argtypes = [I, I, P, P, C.c_int32, P, I, LG, P, P, P, P, P, P, P]

    @staticmethod
    def _rasters(p, side, ad8=None):
        p = np.ascontiguousarray(p, np.int16)
        side = np.ascontiguousarray(side, np.int32)
        return (p, side) if ad8 is None else (p, side, np.ascontiguousarray(ad8, np.float32))

    def moveoutlets(self, p, src, cols, rows, maxdist=50, p_nodata=P_NODATA, src_nodata=SRC_NODATA):
        p, src = self._rasters(p, src)
        ny, nx = p.shape
        x, y = _i32(cols), _i32(rows)
        d = np.zeros_like(x)
        if self._lib.or_moveoutlets(nx, ny, p.ctypes.data, p_nodata, src.ctypes.data, src_nodata, int(maxdist), x.size, x.ctypes.data, y.ctypes.data, d.ctypes.data):
            raise MemoryError("restatement failed")
        return x, y, d

    def moveoutlets_strips(self, p, src, cols, rows, maxdist, cuts, p_nodata=P_NODATA, src_nodata=SRC_NODATA):
        """Strips [cuts[k], cuts[k + 1]) take turns in strip order until a round over all of them makes no iteration; also returns the rounds."""
        p, src = self._rasters(p, src)
        ny, nx = p.shape
        x, y = _i32(cols), _i32(rows)
        d, done = np.zeros_like(x), np.zeros_like(x)
        bounds = [0] + [int(c) for c in cuts] + [ny]
        rounds = 0
        while True:
            rounds += 1
            moved = 0
            for a, b in zip(bounds[:-1], bounds[1:]):
                moved += self._lib.or_moveoutlets_step(nx, ny, p.ctypes.data, p_nodata, src.ctypes.data, src_nodata, int(maxdist), a, b, x.size, x.ctypes.data, y.ctypes.data,
                                                       d.ctypes.data, done.ctypes.data)
            if moved == 0:
                break
        assert done.all()
        return x, y, d, rounds

    def connectdown(self, p, w, ad8, movedist=10, w_nodata=W_NODATA, cap=MAX_ID):
        p, w, ad8 = self._rasters(p, w, ad8)
        ny, nx = p.shape
        n = min(p.size, int(cap) + 1)
        ids, x, y, mx, my, down = (np.zeros(n, np.int32) for _ in range(6))
        amax = np.zeros(n, np.float32)
        k = self._lib.or_connectdown(nx, ny, p.ctypes.data, w.ctypes.data, w_nodata, ad8.ctypes.data, int(movedist), int(cap), ids.ctypes.data, x.ctypes.data, y.ctypes.data,
                                     amax.ctypes.data, mx.ctypes.data, my.ctypes.data, down.ctypes.data)
        if k == -1:
            raise ValueError("watershed id outside 0 .. cap")
        if k < 0:
            raise MemoryError("restatement failed")
        return tuple(a[:k].copy() for a in (ids, x, y, amax, mx, my, down))

    def connectdown_strips(self, p, w, ad8, movedist, cuts, w_nodata=W_NODATA):
        """Every strip's maxima with a table sized by the largest id of the raster, merged in strip order with a strict >, then the walk in turns."""
        p, w, ad8 = self._rasters(p, w, ad8)
        ny, nx = p.shape
        wmax, wmin = C.c_int32(0), C.c_int32(0)
        self._lib.or_id_range(nx, ny, w.ctypes.data, w_nodata, C.addressof(wmax), C.addressof(wmin))
        maxall = wmax.value + 1
        bounds = [0] + [int(c) for c in cuts] + [ny]
        best, locked = {}, set()
        w_real = np.where(np.isnan(ad8), np.int32(w_nodata), w).astype(np.int32)     # the cells that can win by a compare
        for a, b in zip(bounds[:-1], bounds[1:]):
            # the strip's own answer (a NaN on the id's first cell of the strip stands), and its maximum over the cells that are not NaN
            own, real = {}, {}
            for grid, into in ((w, own), (w_real, real)):
                ids, x, y = (np.zeros(maxall, np.int32) for _ in range(3))
                amax = np.zeros(maxall, np.float32)
                k = self._lib.or_argmax_rows(nx, a, b, grid.ctypes.data, w_nodata, ad8.ctypes.data, maxall, ids.ctypes.data, x.ctypes.data, y.ctypes.data, amax.ctypes.data)
                assert k >= 0
                into.update({int(ids[i]): (int(x[i]), int(y[i]), amax[i]) for i in range(k)})
            for i, first in own.items():
                if i not in best:                      # the first strip that holds the id: one rank starts from this cell
                    best[i] = first
                    if np.isnan(first[2]):
                        locked.add(i)                  # x > NaN is false for every x: it is never replaced
                elif i not in locked and i in real and real[i][2] > best[i][2]:
                    best[i] = real[i]
        order = sorted(best)
        ids = np.array(order, np.int32)
        x, y = np.array([best[i][0] for i in order], np.int32), np.array([best[i][1] for i in order], np.int32)
        amax = np.array([best[i][2] for i in order], np.float32)
        mx, my, d, down = x.copy(), y.copy(), np.zeros_like(x), np.zeros_like(x)
        rounds = 0
        while ids.size:
            rounds += 1
            active = 0
            for a, b in zip(bounds[:-1], bounds[1:]):
                while True:
                    k = self._lib.or_walkdown_round(nx, ny, p.ctypes.data, w.ctypes.data, int(movedist), a, b, mx.size, mx.ctypes.data, my.ctypes.data, d.ctypes.data,
                                                    down.ctypes.data)
                    active += k
                    if k == 0:
                        break
            if active == 0:
                break
        return ids, x, y, amax, mx, my, down, rounds


def compile(dirpath):
    lib = os.path.join(str(dirpath), "liboutlets_restate.so")
    subprocess.run(["cc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-o", lib, SRC], check=True)
    return Restatement(lib)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
def cell_centre(gt, cols, rows):
    """tiffIO::globalXYToGeo (src/tiffIO.cpp:593-597) in the same order of operations, as float64."""
    xleft, dlon, ytop, dlat = float(gt[0]), abs(float(gt[1])), float(gt[3]), abs(float(gt[5]))
    cols, rows = np.asarray(cols, np.int64).astype(np.float64), np.asarray(rows, np.int64).astype(np.float64)
    return xleft + dlon / 2.0 + cols * dlon, ytop - dlat / 2.0 - rows * dlat


def to_cells(gt, x, y):
    """tiffIO::geoToGlobalXY (src/tiffIO.cpp:580-588): truncation towards zero."""
    xleft, dlon, ytop, dlat = float(gt[0]), abs(float(gt[1])), float(gt[3]), abs(float(gt[5]))
    return np.trunc((np.asarray(x, np.float64) - xleft) / dlon).astype(np.int32), np.trunc((ytop - np.asarray(y, np.float64)) / dlat).astype(np.int32)


def _num(v):
    return "%.17g" % float(v)


def move_record(gt, ox, oy, ids, rx, ry, dist):
    """The record of a MoveOutletsToStrm run: ox / oy the outlets' own coordinates, rx / ry / dist the result in cells."""
    cx, cy = cell_centre(gt, rx, ry)
    lines = []
    for i in range(len(dist)):
        x, y = (ox[i], oy[i]) if dist[i] < 0 else (cx[i], cy[i])
        lines.append(f"{_num(x)} {_num(y)} id={int(ids[i])} Dist_moved={int(dist[i])}\n")
    return "".join(lines).encode()


def connect_records(gt, res):
    """(the -o record, the -od record) of a ConnectDown result: both carry the same id_down."""
    ids, x, y, amax, mx, my, down = res[:7]
    out = []
    for cols, rows in ((x, y), (mx, my)):
        cx, cy = cell_centre(gt, cols, rows)
        out.append("".join(f"{_num(cx[i])} {_num(cy[i])} id={int(ids[i])} id_down={int(down[i])} ad8={_num(np.float64(amax[i]))}\n" for i in range(len(ids))).encode())
    return tuple(out)


def parse_record(b):
    """[(x, y, {field: text})] of a record's bytes; x and y as float64."""
    rows = []
    for line in bytes(b).decode().splitlines():
        parts = line.split(" ")
        rows.append((float(parts[0]), float(parts[1]), dict(f.split("=", 1) for f in parts[2:])))
    return rows


# ---- inputs of the golden runs ----------------------------------------------------------------------------------------------------------------
def walk_all(p, stream):
    """For every cell the walk of MoveOutletsToStrm without a limit: (steps or -1, final cell, why: 0 stream, 1 p outside 1..8, 2 off the raster)."""
    ny, nx = p.shape
    n = p.size
    steps, final, why = np.zeros(n, np.int64), np.arange(n), np.zeros(n, np.int64)
    for c in range(n):
        cur, k = c, 0
        while True:
            if stream.flat[cur]:
                steps[c], final[c], why[c] = k, cur, 0
                break
            y, x = divmod(cur, nx)
            d = int(p[y, x])
            if not 1 <= d <= 8 or k > n:
                steps[c], final[c], why[c] = -1, cur, 1
                break
            xn, yn = x + DX_[d], y + DY_[d]
            if not (0 <= xn < nx and 0 <= yn < ny):
                steps[c], final[c], why[c] = -1, cur, 2
                break
            cur, k = yn * nx + xn, k + 1
    return steps, final, why


def inputs(name):
    """p, src (int32), w, ad8, gt, geographic of a committed case: p and src of tests/golden/streamnet_<case>.npz and its w_plain, ad8 of the case,
    with what the outlet kinds need planted where the case lacks it: a cell without a direction (p = 0) below an off-stream cell, a path that
    leaves the raster by the east edge, and a second cell that holds its watershed's greatest ad8 (ahead of the first in row-major order)."""
    g = SM.load_golden(name)
    p, src, w = g["p"].copy(), g["src"].astype(np.int32), g["w_plain"].copy()
    ad8 = SM.case_fields(name)["ad8"].copy()
    ny, nx = p.shape
    stream = (src != SRC_NODATA) & (src >= 1)
    plain = ~stream & (p >= 1) & (p <= 8) & (src == 0)
    # p = 0: the receiver r of an off-stream cell u, both off the stream and away from the edges
    for u in np.flatnonzero(plain)[p.size // 5:]:
        y, x = divmod(int(u), nx)
        d = int(p[y, x])
        yr, xr = y + DY_[d], x + DX_[d]
        if 2 <= xr < nx - 2 and 2 <= yr < ny - 2 and plain[yr, xr]:
            p[yr, xr] = 0
            break
    # a path over the east edge: two off-stream cells of one row
    for y in range(ny // 2, ny):
        if not stream[y, nx - 1] and not stream[y, nx - 2]:
            p[y, nx - 2:] = 1
            src[y, nx - 2:] = 0
            break
    # a tie for the maximum: the watershed with the most cells gets its greatest ad8 a second time, on its first cell in row-major order
    ids, counts = np.unique(w[w != W_NODATA], return_counts=True)
    big = int(ids[np.argmax(counts)])
    cells = np.flatnonzero(w.ravel() == big)
    top = cells[np.argmax(ad8.ravel()[cells])]
    ad8.flat[cells[0] if cells[0] != top else cells[-1]] = ad8.flat[top]
    gt = tuple(float(v) for v in g["gt"])
    return p, src, w, ad8, gt, bool(SM.case_fields(name)["geographic"])


def tied_watersheds(w, ad8, w_nodata=W_NODATA):
    """ids whose greatest ad8 is held by two cells or more"""
    out = []
    for i in np.unique(w[w != w_nodata]):
        v = ad8[w == i]
        if np.sum(v == v.max()) >= 2:
            out.append(int(i))
    return out


OUTLET_KINDS = ("on_stream", "one_off", "far", "ends_in_p0", "leaves_raster", "src_nodata", "p_nodata", "off_raster", "twice_a", "twice_b")


def outlet_points(p, src):
    """(cols, rows, ids) of the ten outlets of a golden run, in the order of OUTLET_KINDS; check_outlet_points() says what each must be."""
    ny, nx = p.shape
    stream = (src != SRC_NODATA) & (src >= 1)
    steps, final, why = walk_all(p, stream)
    cells = np.arange(p.size)
    on = np.flatnonzero(stream.ravel())
    pick = {"on_stream": int(on[len(on) // 2])}
    pick["one_off"] = int(np.flatnonzero(steps == 1)[len(np.flatnonzero(steps == 1)) // 2])
    pick["far"] = int(np.argmax(steps))
    ends0 = np.flatnonzero((why == 1) & (final != cells) & (p.ravel()[final] == 0))
    pick["ends_in_p0"] = int(ends0[0])
    leaves = np.flatnonzero((why == 2) & (final != cells))
    pick["leaves_raster"] = int(leaves[0])
    snd = np.flatnonzero((src.ravel() == SRC_NODATA) & (p.ravel() >= 1) & (p.ravel() <= 8))
    pick["src_nodata"] = int(snd[len(snd) // 2])
    pnd = np.flatnonzero(p.ravel() == P_NODATA)
    pick["p_nodata"] = int(pnd[len(pnd) // 2])
    two = np.flatnonzero(steps == 2)
    pick["twice_a"] = pick["twice_b"] = int(two[len(two) // 3])
    cols = [pick[k] % nx if k != "off_raster" else nx + 3 for k in OUTLET_KINDS]
    rows = [pick[k] // nx if k != "off_raster" else ny // 4 for k in OUTLET_KINDS]
    ids = [11, 7, 300, 42, 5, 9001, 64, 2, 13, 12]
    return np.array(cols, np.int32), np.array(rows, np.int32), np.array(ids, np.int32)


def check_outlet_points(p, src, cols, rows):
    """What the golden script asserts of the outlets it runs."""
    ny, nx = p.shape
    stream = (src != SRC_NODATA) & (src >= 1)
    steps, final, why = walk_all(p, stream)
    k = dict(zip(OUTLET_KINDS, (int(r) * nx + int(c) for c, r in zip(cols, rows))))
    assert stream.flat[k["on_stream"]] and steps[k["one_off"]] == 1
    assert steps[k["far"]] > min(MAXDISTS), "no outlet farther away than the smaller maxdist"
    assert why[k["ends_in_p0"]] == 1 and p.flat[final[k["ends_in_p0"]]] == 0 and final[k["ends_in_p0"]] != k["ends_in_p0"]
    assert why[k["leaves_raster"]] == 2 and final[k["leaves_raster"]] != k["leaves_raster"]
    assert src.flat[k["src_nodata"]] == SRC_NODATA and p.flat[k["p_nodata"]] == P_NODATA
    assert not 0 <= cols[OUTLET_KINDS.index("off_raster")] < nx
    assert k["twice_a"] == k["twice_b"] and steps[k["twice_a"]] == 2
    return int(steps[k["far"]])


# ---- hand-built rasters -----------------------------------------------------------------------------------------------------------------------
def small_rasters():
    """name -> (p, w, ad8) for ConnectDown; MoveOutletsToStrm runs on (p, src = (w > 0 cells of ad8 >= 3)) of the same rasters: small_src()."""
    out = {}
    f32 = np.float32

    def blank(ny, nx, pdir=7):
        return np.full((ny, nx), pdir, np.int16), np.full((ny, nx), W_NODATA, np.int32), np.zeros((ny, nx), f32)

    p, w, a = blank(1, 1); w[0, 0] = 3; a[0, 0] = 2.5; out["one_cell"] = (p, w, a)
    p, w, a = blank(1, 9, 1); w[0, :] = [1, 1, 2, 2, 2, W_NODATA, 4, 4, 1]; a[0, :] = [1, 2, 5, 9, 3, 7, 1, 1, 8]; out["one_row"] = (p, w, a)
    p, w, a = blank(9, 1); w[:, 0] = [1, 1, 2, 2, 2, W_NODATA, 4, 4, 1]; a[:, 0] = [1, 2, 5, 9, 3, 7, 1, 1, 8]; out["one_column"] = (p, w, a)
    p, w, a = blank(6, 7); w[:] = 5; w[2, 3] = 9; a[:] = np.arange(42, dtype=f32).reshape(6, 7); out["single_cell_watershed"] = (p, w, a)
    p, w, a = blank(6, 7); w[:3] = 0; w[3:] = 2; a[:] = np.arange(42, dtype=f32).reshape(6, 7)[::-1]; out["id_zero"] = (p, w, a)
    p, w, a = blank(5, 8); w[:] = 1; w[4, 7] = 40; a[:] = 1; a[4, 7] = 0.5; out["largest_id_last_cell"] = (p, w, a)
    # 40 x 64 = 2560 cells: the two maxima of id 6 lie 2304 cells apart, in different workgroups of 2048 cells
    p, w, a = blank(40, 64); w[:] = 6; w[:, 32:] = 7; a[:] = 1; a[2, 5] = 50; a[38, 5] = 50; a[20, 40] = 9; a[21, 40] = 9; out["tie_far_apart"] = (p, w, a)
    p, w, a = blank(4, 64); w[:] = 2; a[:] = 1; a[0, 17] = 8; a[0, 19] = 8; out["tie_in_one_wave"] = (p, w, a)
    p, w, a = blank(4, 10); w[:2] = 1; w[2:] = 2; a[:] = -1; a[0, 3] = -0.0; a[1, 4] = 0.0; a[2, 3] = 0.0; a[3, 4] = -0.0; out["minus_zero"] = (p, w, a)
    p, w, a = blank(4, 10); w[:2] = 1; w[2:] = 2; a[:] = 3; a[0, 0] = np.nan; a[1, 5] = 7; a[2, 4] = np.nan; a[3, 2] = 6; out["nan_first_and_later"] = (p, w, a)
    p, w, a = blank(5, 6); a[:] = 4; out["all_nodata"] = (p, w, a)
    # a NaN on the first cell of a ROW that is not the id's first cell: a strip that starts there must not take it for the strip's answer
    p, w, a = blank(4, 6); w[:] = 1; a[:] = 1; a[2, 0] = np.nan; a[2, 3] = 10; a[3, 1] = 10; w[0, 5] = 2; w[3, 5] = 2; a[0, 5] = np.nan; a[3, 5] = 99
    out["nan_heads_a_strip"] = (p, w, a)
    p, w, a = blank(12, 20, 8); yy, xx = np.mgrid[0:12, 0:20]; w[:] = (yy + xx) % 2 + 1; a[:] = ((yy * 7 + xx * 13) % 31).astype(f32); out["checkerboard"] = (p, w, a)
    # the only stream cell at column 68 of a row of 70: outlets farther than 50 steps from it (the committed cases have none beyond 19), one at 50
    p, w, a = blank(1, 70, 1); w[:] = 1; a[0, 68] = 5; out["long_row"] = (p, w, a)
    for name, (p, w, a) in out.items():
        ny, nx = p.shape
        if ny > 2 and nx > 2:
            p[ny // 2, nx // 2] = P_NODATA          # a walk that stops early
            p[:, 0] = 5                              # and walks that leave by the west edge
    return out


def small_src(w, ad8):
    return np.where(w == W_NODATA, SRC_NODATA, np.where(np.nan_to_num(ad8) >= 3, 1, 0)).astype(np.int32)


def small_outlets(p):
    """cell (cols, rows, ids): every third cell, one off the raster, one twice"""
    ny, nx = p.shape
    c = np.arange(0, p.size, 3)
    cols, rows = list(c % nx) + [-1, int(c[0] % nx)], list(c // nx) + [0, int(c[0] // nx)]
    return np.array(cols, np.int32), np.array(rows, np.int32), np.arange(1, len(cols) + 1, dtype=np.int32)


def load_golden(name):
    g = np.load(os.path.join(HERE, "golden", f"outlets_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}
