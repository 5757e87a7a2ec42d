"""Golden vectors for EditRaster: runs the REAL reference tool.  Build container only, after build() has left the reference's common objects in oracle/_ref/obj:

    python tests/golden/make_golden_editraster.py

EditRaster.cpp and EditRastermn.cpp are compiled unmodified into a temporary directory with make_golden_d8rev.build_tool; nothing is written under oracle/.
editraster_small.npz holds, for every raster and change file of editraster_model.cases(): the input ("in/<case>", "nodata/<case>"), the change file's text
("changes/<case>/<file>"), the real tool's output raster ("out/<case>/<file>") and what it printed ("stdout/<case>/<file>", the number of the "Compute time"
line replaced by "T" - it is the one thing that differs from run to run; the tool runs in the temporary directory on relative file names).

The script ASSERTS what the fixtures are there to show: the output's nodata tag is -32768; every output equals editraster_model.edit() on the records
editraster_model.scan_changes() finds, and the "Process: 0 changing" lines equal process_lines(); a duplicate cell takes the LAST value; a point on the left
and top edges lands in cell (0, 0); a point less than one cell left of or above the raster lands in column / row 0 too - (int) truncates towards zero - and
IS applied by the reference; a point on the right or bottom edge is off the raster; the valid lines after a malformed one are not applied.
"""
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import editraster_model as M  # noqa: E402
import make_golden_d8rev as R  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def run(exe, d, a, nodata, text):
    gt = M.geotransform(a.shape[0])
    for f in ("out.tif",):
        if os.path.exists(os.path.join(d, f)):
            os.remove(os.path.join(d, f))
    T.write_raster(os.path.join(d, "in.tif"), a, int(nodata), geotransform=gt)
    with open(os.path.join(d, "changes.txt"), "w") as fh:
        fh.write(text)
    stdout, _, _ = O.run_ref(exe, ["-in", "in.tif", "-out", "out.tif", "-changes", "changes.txt"], 1, cwd=d)
    out, info = T.read_raster(os.path.join(d, "out.tif"), np.int16)
    assert float(info["nodata"]) == -32768.0 and out.dtype == np.int16, info
    return out, re.sub(r"(Compute time: )[0-9.eE+-]+", r"\1T", stdout)


if __name__ == "__main__":
    O.build()
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_tool(tmp, "editraster", ("EditRaster", "EditRastermn"))
        for name, (a, nodata, files) in M.cases().items():
            ny, nx = a.shape
            gt = M.geotransform(ny)
            data[f"in/{name}"], data[f"nodata/{name}"] = a, np.int64(nodata)
            plain = np.where(a == nodata, M.OUT_NODATA, a).astype(np.int16)
            for fname, text in files.items():
                out, stdout = run(exe, tmp, a, nodata, text)
                x, y, v = M.scan_changes(text)
                c, r = M.cells(x, y, gt)
                assert np.array_equal(out, M.edit(a, nodata, c, r, v)), f"{name} {fname}: the tool differs from the model"
                lines = [ln for ln in stdout.splitlines() if ln.startswith("Process:")]
                assert lines == M.process_lines(x, y, v, gt, a.shape, as_reference=True), f"{name} {fname}: {lines}"
                # the reference's rank after a negative value: editraster_model.process_lines
                assert ("Compute time: T" in stdout) == (len(v) == 0 or v[-1] >= 0), f"{name} {fname}: {stdout}"
                if fname == "none":
                    assert np.array_equal(out, plain) and not lines
                if fname == "dup":
                    assert out[ny - 1, nx - 1] == 13 and len(lines) == 3
                if fname == "edges":
                    # 21 on the edges -> (0, 0); 22 left of the raster -> column 0 of the last row; 23 above it -> row 0 of the last column; 24, 25, 26 off
                    # (on the 1 x 1 raster the three are one cell, and the last one holds)
                    assert len(lines) == 3 and out[ny - 1, 0] == (22 if nx > 1 else 23) and out[0, nx - 1] == 23 and out[0, 0] == (21 if nx > 1 else 23)
                    assert not np.isin(out, (24, 25, 26)).any()
                if fname == "malformed":
                    assert len(x) == 1 and out[ny - 1, nx - 1] == 31 and not np.isin(out, (32, 33)).any()
                if fname == "values":
                    assert len(x) == 3 and out[ny - 1, nx - 1] == (32767 if nx > 1 else -5) and out[0, 0] == -5
                data[f"changes/{name}/{fname}"] = np.array(text)
                data[f"out/{name}/{fname}"] = out
                data[f"stdout/{name}/{fname}"] = np.array(stdout)
                print(name, fname, a.shape, len(x), "records,", len(lines), "applied")
        print(stdout)
    np.savez_compressed(os.path.join(OUT, "editraster_small.npz"), **data)
    print("file bytes", os.path.getsize(os.path.join(OUT, "editraster_small.npz")))
