"""CatchHydroGeo's and InunDepth's semantics as a plain C program (tests/hand/hand_restate.c): one raster scan with running sums, the CSV
readers, the interpolation and both table writers.

    compile(dirpath)   builds the shared library with `cc` into dirpath (a pytest temporary directory) and returns a Restatement
    Restatement.chg_sums(hand, cat, slp, dxc, dyc, ids, stages)   (count, surface, bed, volume, catcharea)
    Restatement.chg_tool(..., listfile, stagefile, tablefile)      the whole tool: read the two text files, scan, write the table
    Restatement.inun_depths(fcfile, hpfile)                        (ids, flow, depth, catcharea)
    Restatement.inun_map / inun_area / inun_write_depths

tests/test_hand_restatement.py holds it to every golden of tests/golden/hand_*.npz byte for byte, so that the GPU tests can use it at sizes
the goldens do not cover.  voronoi() and the exact-sum helpers of the GPU tests live here too.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hand", "hand_restate.c")
HAND_NODATA = -3.4028235e38   # MISSINGFLOAT: what dinfdistdown writes
SLP_NODATA = -1.0
CATCH_NODATA = -9999
MASK_NODATA = -32768
MAP_NODATA = np.float32(-3.0e38)
U = 2.0 ** -53
CAP = 1 << 17


def _f64(a, n):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), (n,)))


class Restatement:
    def __init__(self, lib_path):
        self._lib = C.CDLL(lib_path)
        for name in ("chg_sums", "chg_read_list", "chg_read_stages", "chg_write_table", "inun_depths", "inun_map", "inun_area", "inun_write_depths"):
            getattr(self._lib, name).restype = C.c_int
        P, I, F = C.c_void_p, C.c_int, C.c_float
        self._lib.chg_sums.argtypes = [I, I, P, F, P, C.c_int32, P, F, P, P, P, I, P, I, P, P, P, P, P]
        self._lib.chg_read_list.argtypes = [C.c_char_p, I, P, P, P, P, P, P]
        self._lib.chg_read_stages.argtypes = [C.c_char_p, I, P, P]
        self._lib.chg_write_table.argtypes = [C.c_char_p, P, P, P, P, I, P, I, P, P, P, P, P]
        self._lib.inun_depths.argtypes = [C.c_char_p, C.c_char_p, I, P, P, P, P, P]
        self._lib.inun_map.argtypes = [I, I, P, F, P, C.c_int32, P, C.c_int16, P, P, I, P]
        self._lib.inun_area.argtypes = [I, I, P, F, P, C.c_int32, P, P, P, P, I, P]
        self._lib.inun_write_depths.argtypes = [C.c_char_p, P, P, P, P, P, I]

    def chg_sums(self, hand, cat, slp, dxc, dyc, ids, stages, hand_nodata=HAND_NODATA, catch_nodata=CATCH_NODATA, slp_nodata=SLP_NODATA):
        ny, nx = hand.shape
        hand, slp = np.ascontiguousarray(hand, np.float32), np.ascontiguousarray(slp, np.float32)
        cat, ids = np.ascontiguousarray(cat, np.int32), np.ascontiguousarray(ids, np.int32)
        dxc, dyc, stages = _f64(dxc, ny), _f64(dyc, ny), np.ascontiguousarray(stages, np.float64)
        nc, nh = ids.size, stages.size
        count = np.zeros((nh, nc), np.int32)
        surf, bed, vol = (np.zeros((nh, nc), np.float64) for _ in range(3))
        carea = np.zeros(nc, np.float64)
        rc = self._lib.chg_sums(nx, ny, hand.ctypes.data, float(hand_nodata), cat.ctypes.data, int(catch_nodata), slp.ctypes.data, float(slp_nodata), dxc.ctypes.data,
                                dyc.ctypes.data, ids.ctypes.data, nc, stages.ctypes.data, nh, count.ctypes.data, surf.ctypes.data, bed.ctypes.data, vol.ctypes.data,
                                carea.ctypes.data)
        assert rc == 0
        return count, surf, bed, vol, carea

    def read_list(self, path):
        ids = np.zeros(CAP, np.int32)
        slope, length, mann = (np.zeros(CAP, np.float64) for _ in range(3))
        n, four = C.c_int(0), C.c_int(0)
        rc = self._lib.chg_read_list(os.fsencode(path), CAP, ids.ctypes.data, slope.ctypes.data, length.ctypes.data, mann.ctypes.data, C.addressof(n), C.addressof(four))
        if rc != 0:
            raise ValueError(rc)
        return ids[:n.value].copy(), slope[:n.value].copy(), length[:n.value].copy(), mann[:n.value].copy()

    def read_stages(self, path):
        st = np.zeros(CAP, np.float64)
        n = C.c_int(0)
        rc = self._lib.chg_read_stages(os.fsencode(path), CAP, st.ctypes.data, C.addressof(n))
        if rc != 0:
            raise ValueError(rc)
        return st[:n.value].copy()

    def write_table(self, path, ids, slope, length, mann, stages, count, surf, bed, vol, carea):
        arrs = [np.ascontiguousarray(ids, np.int32)] + [np.ascontiguousarray(a, np.float64) for a in (slope, length, mann)]
        stages = np.ascontiguousarray(stages, np.float64)
        outs = [np.ascontiguousarray(count, np.int32)] + [np.ascontiguousarray(a, np.float64) for a in (surf, bed, vol, carea)]
        rc = self._lib.chg_write_table(os.fsencode(path), *(a.ctypes.data for a in arrs), arrs[0].size, stages.ctypes.data, stages.size, *(a.ctypes.data for a in outs))
        assert rc == 0

    def chg_tool(self, hand, cat, slp, dxc, dyc, listfile, stagefile, tablefile, **nodata):
        ids, slope, length, mann = self.read_list(listfile)
        stages = self.read_stages(stagefile)
        sums = self.chg_sums(hand, cat, slp, dxc, dyc, ids, stages, **nodata)
        self.write_table(tablefile, ids, slope, length, mann, stages, *sums)
        return sums

    def inun_depths(self, fcfile, hpfile):
        ids = np.zeros(CAP, np.int32)
        flow = np.zeros(CAP, np.float64)
        depth, carea = np.zeros(CAP, np.float32), np.zeros(CAP, np.float32)
        n = C.c_int(0)
        rc = self._lib.inun_depths(os.fsencode(fcfile), os.fsencode(hpfile), CAP, ids.ctypes.data, flow.ctypes.data, depth.ctypes.data, carea.ctypes.data, C.addressof(n))
        if rc != 0:
            raise ValueError(rc)
        return ids[:n.value].copy(), flow[:n.value].copy(), depth[:n.value].copy(), carea[:n.value].copy()

    def inun_map(self, hand, cat, ids, depth, mask=None, hand_nodata=HAND_NODATA, catch_nodata=CATCH_NODATA, mask_nodata=MASK_NODATA):
        ny, nx = hand.shape
        hand, cat = np.ascontiguousarray(hand, np.float32), np.ascontiguousarray(cat, np.int32)
        ids, depth = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(depth, np.float32)
        m = None if mask is None else np.ascontiguousarray(mask, np.int16)
        out = np.empty((ny, nx), np.float32)
        rc = self._lib.inun_map(nx, ny, hand.ctypes.data, float(hand_nodata), cat.ctypes.data, int(catch_nodata), None if m is None else m.ctypes.data, int(mask_nodata),
                                ids.ctypes.data, depth.ctypes.data, ids.size, out.ctypes.data)
        assert rc == 0
        return out

    def inun_area(self, hand, cat, dxc, dyc, ids, depth, hand_nodata=HAND_NODATA, catch_nodata=CATCH_NODATA):
        ny, nx = hand.shape
        hand, cat = np.ascontiguousarray(hand, np.float32), np.ascontiguousarray(cat, np.int32)
        ids, depth = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(depth, np.float32)
        dxc, dyc = _f64(dxc, ny), _f64(dyc, ny)
        out = np.zeros(ids.size, np.float32)
        rc = self._lib.inun_area(nx, ny, hand.ctypes.data, float(hand_nodata), cat.ctypes.data, int(catch_nodata), dxc.ctypes.data, dyc.ctypes.data, ids.ctypes.data,
                                 depth.ctypes.data, ids.size, out.ctypes.data)
        assert rc == 0
        return out

    def write_depths(self, path, ids, flow, depth, area, carea):
        a = [np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(flow, np.float64)] + [np.ascontiguousarray(x, np.float32) for x in (depth, area, carea)]
        assert self._lib.inun_write_depths(os.fsencode(path), *(x.ctypes.data for x in a), a[0].size) == 0


def compile(dirpath):
    lib = os.path.join(str(dirpath), "libhand_restate.so")
    subprocess.run(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-o", lib, SRC, "-lm"], check=True)
    return Restatement(lib)


def load_golden(name):
    g = np.load(os.path.join(HERE, "golden", f"hand_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def golden_names():
    return sorted(f[len("hand_"):-len(".npz")] for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("hand_") and f.endswith(".npz"))


def text_of(a):
    """A byte-string array of a golden as bytes."""
    return bytes(np.asarray(a).tobytes()) if np.asarray(a).dtype == np.uint8 else bytes(a.item())


def voronoi(ny, nx, nseeds, seed, ids=None):
    """Seeded Voronoi labels: (ny, nx) int32 of ids[nearest seed] (default 1..nseeds)."""
    rng = np.random.default_rng(seed)
    sy, sx = rng.uniform(0, ny, nseeds), rng.uniform(0, nx, nseeds)
    yy, xx = np.mgrid[0:ny, 0:nx]
    best = np.full((ny, nx), np.inf)
    lab = np.zeros((ny, nx), np.int64)
    for s in range(nseeds):
        d = (yy - sy[s]) ** 2 + (xx - sx[s]) ** 2
        m = d < best
        best[m], lab[m] = d[m], s
    ids = np.arange(1, nseeds + 1) if ids is None else np.asarray(ids)
    return ids[lab].astype(np.int32)


def gamma(n):
    """Higham's bound factor for a sum of n fp64 terms taken in any order."""
    return 0.0 if n <= 1 else (n - 1) * U / (1.0 - (n - 1) * U)


def exact_sums(hand, cat, slp, dxc, dyc, ids, stages, hand_nodata=HAND_NODATA, catch_nodata=CATCH_NODATA, slp_nodata=SLP_NODATA):
    """Per table entry: the contributing-cell count n, math.fsum of the terms and of their magnitudes, the terms evaluated as the reference
    evaluates them (float32 product and square root for the bed factor, fp64 elsewhere).  Returns dicts keyed 'surface' / 'bed' / 'volume' of
    (exact, sumabs) arrays [nh][nc], the counts [nh][nc], and (exact, sumabs, n) of the catchment areas."""
    ny, nx = hand.shape
    ids, stages = np.asarray(ids, np.int32), np.asarray(stages, np.float64)
    nc, nh = ids.size, stages.size
    dxc, dyc = _f64(dxc, ny), _f64(dyc, ny)
    area = np.repeat((dxc * dyc)[:, None], nx, 1)
    win = {int(v): i for i, v in enumerate(ids)}                       # last wins
    idx = np.full(cat.shape, -1, np.int64)
    for v in np.unique(cat):
        if int(v) in win:
            idx[cat == v] = win[int(v)]
    idx[np.abs((cat.astype(np.int64) - int(catch_nodata))) < 1] = -1
    h32, s32 = hand.astype(np.float32), slp.astype(np.float32)
    nd = (np.abs((h32 - np.float32(hand_nodata)).astype(np.float32)) < np.float32(1e-5)) | (np.abs((s32 - np.float32(slp_nodata)).astype(np.float32)) < np.float32(1e-5))
    root = np.sqrt((np.float32(1) + s32 * s32).astype(np.float32)).astype(np.float32).astype(np.float64)
    h64 = h32.astype(np.float64)
    zero = np.abs(h64) < 0.000001
    out = {k: (np.zeros((nh, nc)), np.zeros((nh, nc))) for k in ("surface", "bed", "volume")}
    count = np.zeros((nh, nc), np.int64)
    ca = (np.zeros(nc), np.zeros(nc), np.zeros(nc, np.int64))
    for c in np.unique(idx[idx >= 0]):
        m = idx == c
        a = area[m]
        ca[0][c], ca[1][c], ca[2][c] = math.fsum(a), math.fsum(np.abs(a)), a.size
        ok = ~nd[m]
        a, hh, rr, zz = a[ok], h64[m][ok], root[m][ok], zero[m][ok]
        for k in range(nh):
            w = (hh < stages[k]) | zz
            count[k, c] = int(w.sum())
            terms = {"surface": a[w], "bed": a[w] * rr[w], "volume": (stages[k] - hh[w]) * a[w]}
            for key, t in terms.items():
                out[key][0][k, c], out[key][1][k, c] = math.fsum(t), math.fsum(np.abs(t))
    return out, count, ca
