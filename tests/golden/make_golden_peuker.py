"""Golden vectors for PeukerDouglas (src/PeukerDouglas.cpp): runs the REAL reference tool.  Build container only, after build() has left the reference's
common objects in oracle/_ref/obj:

    python tests/golden/make_golden_peuker.py

The reference tool is compiled into a temporary directory with make_golden_d8rev.build_tool; nothing is written under oracle/.
peuker_<case>.npz, for the five committed cases (the runs of peuker_model.golden_runs): ss of fel and of dem with the default weights, of dem with five
-par settings (a zero side weight, a zero diagonal weight, the centre alone, no centre, all zero - 0/0, no flagged cell), and for `holes` and
`fourway_mask` of fel with nodata rewritten to +9999 (the first cell of a group starts the maximum without a nodata test, so the sign of the nodata
value matters next to holes).  Every input is run on 3 ranks as well and the script ASSERTS that the output equals the 1-rank output.
peuker_patho.npz: the generators of tests/pathological.py (peuker_model.PATHO) at their own sizes, nodata -9999, default weights, one rank.
The script also asserts that the restatement (tests/peuker/peuker_restate.cpp) reproduces every array.  ss is stored as int8, compressed.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_d8rev as R  # noqa: E402
import peuker_model as M  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def run(exe, d, z, nodata, weights, ranks=1):
    f = lambda s: os.path.join(d, s)  # noqa: E731
    ny = z.shape[0]
    T.write_raster(f("fel.tif"), z, float(nodata), geotransform=(1000.0, 30.0, 0.0, 5000.0 + 30.0 * ny, 0.0, -30.0))
    if os.path.exists(f("ss.tif")):
        os.remove(f("ss.tif"))
    O.run_ref(exe, ["-fel", f("fel.tif"), "-ss", f("ss.tif"), "-par", *[repr(float(w)) for w in weights]], ranks)
    ss, info = T.read_raster(f("ss.tif"), np.int16)
    assert M.tiff_sample_type(f("ss.tif")) == (16, 2) and float(info["nodata"]) == -2.0, (M.tiff_sample_type(f("ss.tif")), info["nodata"])
    assert set(np.unique(ss).tolist()) <= {0, 1}
    return ss


if __name__ == "__main__":
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_tool(tmp, "peukerdouglas", ("PeukerDouglas", "PeukerDouglasmn"))
        restate = M.compile(tmp)
        for c in M.CASES:
            res = {}
            for key, z, nd, w in M.golden_runs(c):
                ss = run(exe, tmp, z, nd, w)
                ss3 = run(exe, tmp, z, nd, w, ranks=3)
                assert np.array_equal(ss, ss3), f"{c} {key}: the 3-rank output differs from the 1-rank output in {int(np.sum(ss != ss3))} cells"
                assert np.array_equal(ss, restate.run(z, nd, w)), f"{c} {key}: the restatement differs from the reference"
                res[key] = ss.astype(np.int8)
                print(c, key, z.shape, "flagged", int(ss.sum()), f"({100.0 * ss.mean():.1f} %)", "3 ranks: same")
            np.savez_compressed(os.path.join(OUT, f"peuker_{c}.npz"), **res)
        res = {}
        for name, z in M.patho_inputs():
            ss = run(exe, tmp, z, -9999.0, M.DEFAULT)
            assert np.array_equal(ss, restate.run(z, -9999.0, M.DEFAULT)), f"{name}: the restatement differs from the reference"
            res[name] = ss.astype(np.int8)
            print("patho", name, z.shape, "flagged", int(ss.sum()))
        np.savez_compressed(os.path.join(OUT, "peuker_patho.npz"), **res)
