"""PeukerDouglas' semantics as a serial C++ program (tests/peuker/peuker_restate.cpp): the reference's loops as written - smoothing pass, copy back, the
sequential scan over the 2x2 groups that clears flags in scan order - on one rank.

    compile(dirpath)            builds the shared library with g++ into dirpath (a pytest temporary directory) and returns a Restatement
    Restatement.run(fel, ...)   ss (int16), optionally the smoothed grid

tests/test_peuker_restatement.py holds it to every array of tests/golden/peuker_*.npz exactly, so that the GPU tests can use it at sizes the goldens
do not cover.  The runs the goldens hold, and the inputs they were made from, are listed here too (golden_runs / patho_inputs): the script that
makes the goldens and the tests that read them walk the same lists.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "peuker", "peuker_restate.cpp")
GOLDEN = os.path.join(HERE, "golden")
CASES = ("fourway_mask", "geographic", "holes", "plain", "rect_dxdy")
FEL_NODATA = np.float32(-3.0e38)
DEFAULT = (0.4, 0.1, 0.05)
PARS = ((0.5, 0.125, 0.0), (0.5, 0.0, 0.125), (1.0, 0.0, 0.0), (0.0, 1.0, 1.0), (0.0, 0.0, 0.0))   # the -par settings of the goldens, run on dem
POSITIVE = ("holes", "fourway_mask")   # cases whose fel is also run with nodata rewritten to +9999
PATHO = ("plane", "ramp_diag", "ramp_shallow", "checkerboard_pits", "spiral", "one_row", "one_column", "two_rows", "all_nodata", "one_data_cell", "nan_cells",
         "+inf_cells", "-inf_cells")   # generators of tests/pathological.py, at their own sizes, nodata -9999


def golden_runs(name):
    """[(key, raster, nodata, weights)] of the runs peuker_<name>.npz holds, from case_<name>.npz"""
    g = np.load(os.path.join(GOLDEN, f"case_{name}.npz"))
    fel, dem, dem_nd = g["fel"], g["dem"], np.float32(g["nodata"])
    runs = [("fel_default", fel, FEL_NODATA, DEFAULT), ("dem_default", dem, dem_nd, DEFAULT)]
    runs += [(f"dem_par{i}", dem, dem_nd, w) for i, w in enumerate(PARS)]
    if name in POSITIVE:
        runs.append(("fel_pos9999", np.where(fel == FEL_NODATA, np.float32(9999.0), fel).astype(np.float32), np.float32(9999.0), DEFAULT))
    return runs


def patho_inputs():
    """[(name, raster)] of the runs peuker_patho.npz holds (nodata -9999, default weights)"""
    import pathological as PG
    from oracle import oracle as O

    return [(n, np.ascontiguousarray(PG.CASES[n](O), np.float32)) for n in PATHO]


def load_golden(name):
    """{key: ss int16} of peuker_<name>.npz (stored as int8)"""
    return {k: v.astype(np.int16) for k, v in np.load(os.path.join(GOLDEN, f"peuker_{name}.npz")).items()}


def tiff_sample_type(path):
    """(BitsPerSample, SampleFormat) of the first image of a TIFF or BigTIFF file: (16, 2) is int16"""
    import struct

    b = open(path, "rb").read()
    e = "<" if b[:2] == b"II" else ">"
    big = struct.unpack(e + "H", b[2:4])[0] == 43
    off = struct.unpack(e + "Q", b[8:16])[0] if big else struct.unpack(e + "I", b[4:8])[0]
    n = struct.unpack(e + ("Q" if big else "H"), b[off:off + (8 if big else 2)])[0]
    off += 8 if big else 2
    tags = {}
    for i in range(n):
        ent = b[off + i * (20 if big else 12):off + (i + 1) * (20 if big else 12)]
        tag, typ = struct.unpack(e + "HH", ent[:4])
        if typ == 3:   # SHORT, count 1: the value sits in the entry
            tags[tag] = struct.unpack(e + "H", ent[12:14] if big else ent[8:10])[0]
    return tags.get(258), tags.get(339, 1)


class Restatement:
    def __init__(self, lib_path):
        self._lib = C.CDLL(lib_path)
        self._lib.pk_run.restype = None
        self._lib.pk_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(self, fel, nodata=FEL_NODATA, weights=DEFAULT, smoothed=False):
        fel = np.ascontiguousarray(fel, np.float32)
        ny, nx = fel.shape
        p = np.array(weights, np.float32)
        ss = np.zeros((ny, nx), np.int16)
        sm = np.zeros((ny, nx), np.float32) if smoothed else None
        self._lib.pk_run(nx, ny, fel.ctypes.data, float(np.float32(nodata)), p.ctypes.data, ss.ctypes.data, sm.ctypes.data if smoothed else None)
        return (ss, sm) if smoothed else ss


def compile(dirpath):
    lib = os.path.join(str(dirpath), "peuker_restate.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", lib], check=True)
    return Restatement(lib)
