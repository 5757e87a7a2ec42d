"""Golden vectors for RetLimFlow (src/RetlimFlow.cpp) and DinfAvalanche (src/DinfAvalanche.cpp): runs the REAL reference tools on the
D-infinity angles and pit-filled elevations of the committed cases.  Build container only, after build() has left the reference's common
objects in oracle/_ref/obj:

    python tests/golden/make_golden_aval.py

The reference tools are compiled into a temporary directory (the flags of oracle/Makefile's REFFLAGS, linked against oracle/_ref/obj);
nothing is written under oracle/.  aval_<case>.npz holds the inputs - ang with a few interior cells without a direction (-1) and without
an angle (nodata), fel with a few nodata cells under valid angles, wg and rc with nodata cells and regions where rc > wg (the clamp), ass
with source patches on steep ground plus single-cell sources, per-row cell sizes, the geotransform {xleftedge, ytopedge, dlon, dlat} -
and the reference's rasters: qrl, and rz / dfs for the path and -direct modes with the default and one other (thresh, alpha)
(tests/aval_model.variants()).  The files are named aval_*.npz, not case_*.npz: conftest.golden_cases() takes every case_*.npz as a case.
For three cases the reference's 3-rank run must equal its 1-rank run.  The script also prints the share of cells the C restatement
marks as tainted (tests/aval_model.py): it has to stay below 1 % of the cells with rz data.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aval_model as M  # noqa: E402
import taudem_amd as T  # noqa: E402  (raster file IO only)
from oracle import oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
REF_SRC = "/root/reference/src"
MPI_ROOT = "/opt/conda"
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
CASES = ("plain", "holes", "rect_dxdy", "geographic", "fourway_mask")


def build_tool(d, sources, name):
    """Compiles a reference tool into directory d; returns the executable."""
    inc = ["-Igdal_shim", f"-I{os.path.join(ROOT, 'oracle', '_ref', 'mpiinc')}", f"-I{REF_SRC}"]
    flags = ["-std=c++17", "-O3", "-w"]   # oracle/Makefile REFFLAGS
    objs = []
    for s in sources:
        o = os.path.join(d, s + ".o")
        subprocess.run(["g++"] + flags + inc + ["-c", os.path.join(REF_SRC, s + ".cpp"), "-o", o], check=True, cwd=os.path.join(ROOT, "oracle"))
        objs.append(o)
    common = [os.path.join(OBJ, f + ".o") for f in ("commonLib", "tiffIO", "ReadOutlets", "shim", "geotiff", "outlets")]
    exe = os.path.join(d, name)
    subprocess.run(["g++"] + objs + common + [f"{MPI_ROOT}/lib/libmpi.so", f"-Wl,-rpath,/usr/lib/x86_64-linux-gnu:{MPI_ROOT}/lib", "-Wl,--allow-shlib-undefined",
                                              "-lz", "-o", exe], check=True)
    return exe


def inputs(name):
    g = np.load(os.path.join(OUT, f"case_{name}.npz"))
    ang = g["ang"].copy()
    fel = g["fel"].copy()
    ny, nx = ang.shape
    dxc, dyc = g["dxc"], g["dyc"]
    rng = np.random.default_rng(4100 + nx + ny)
    inner = np.zeros((ny, nx), bool)
    inner[2:-2, 2:-2] = True
    valid = ang > -1e30
    ang[inner & valid & (rng.random((ny, nx)) < 0.003)] = -1.0                # interior cells without a direction (sends east where atan2(dy, dx) > 1)
    ang[inner & (rng.random((ny, nx)) < 0.002)] = M.ANG_NODATA                # interior cells without an angle
    valid = ang > -1e30
    fel[(rng.random((ny, nx)) < 0.004) & valid] = M.FEL_NODATA                # nodata elevations under valid angles: not evaluated, still release
    # RetLimFlow: rainfall excess in steps of 1/8, retention mostly below it, larger in blocks (the clamp), a few nodata cells in both
    wg = (rng.integers(0, 33, (ny, nx)) / 8.0).astype(np.float32)
    rc = (rng.integers(0, 9, (ny, nx)) / 8.0).astype(np.float32)
    for _ in range(6):
        j, i = int(rng.integers(0, ny - 12)), int(rng.integers(0, nx - 12))
        rc[j:j + 12, i:i + 12] += 40.0
    wg[rng.random((ny, nx)) < 0.0015] = M.WG_NODATA
    rc[rng.random((ny, nx)) < 0.0015] = M.RC_NODATA
    return g, ang, fel, wg, rc


def sources(g, fel, seed):
    """ass for one seed: source patches where the ground is steep, single cells anywhere, a few nodata cells."""
    ny, nx = fel.shape
    rng = np.random.default_rng(seed)
    f = np.where(fel > -1e30, fel, np.nan)
    gy, gx = np.gradient(f)
    slope = np.nan_to_num(np.degrees(np.arctan(np.hypot(gx / g["dxc"][:, None], gy / g["dyc"][:, None]))), nan=0.0)
    ass = np.zeros((ny, nx), np.int16)
    steep = np.argwhere(slope > np.percentile(slope, 85))
    for j, i in steep[rng.choice(len(steep), 5, replace=False)]:
        ass[max(j - 1, 0):j + 2, max(i - 1, 0):i + 3] = 1
    ass[rng.random((ny, nx)) < 0.004] = 2
    ass[rng.random((ny, nx)) < 0.002] = M.ASS_NODATA
    return ass


def choose_sources(R, g, ang, fel, geo, geographic):
    """The first seed whose tainted share (the C restatement alone, tests/aval_model.py) stays below 0.8 % of the cells with rz data in all four
    runs and leaves at least 150 such cells: near-ties between two paths from one source are a property of the terrain, and a fixture in
    which they taint more than 1 % of the runout would hide a broken kernel behind the mask."""
    for seed in range(7000, 9000):
        ass = sources(g, fel, seed)
        worst, least = 0.0, 1 << 30
        for _, direct, ta in M.variants():
            rz, _, taint = R.dinfavalanche(ang, fel, ass, thresh=ta[0], alpha=ta[1], direct=direct, dxc=g["dxc"], dyc=g["dyc"], geo=geo, geographic=geographic)
            has = int((rz > -1e30).sum())
            worst, least = max(worst, taint.sum() / max(has, 1)), min(least, has)
        if worst <= 0.008 and least >= 150:
            return ass, seed
    raise RuntimeError("no seed keeps the tainted share below the limit")


def make(exes, R, name, check_ranks=0):
    g, ang, fel, wg, rc = inputs(name)
    ny, nx = ang.shape
    dx, dy, geographic = float(g["dx"]), float(g["dy"]), bool(g["geographic"])
    gt = (-111.9, dx, 0.0, 41.9, 0.0, -dy) if geographic else (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)
    ass, seed = choose_sources(R, g, ang, fel, (gt[0], gt[3], dx, dy), geographic)
    res = {"ang": ang, "fel": fel, "wg": wg, "rc": rc, "ass": ass, "dxc": g["dxc"], "dyc": g["dyc"], "geo": np.array([gt[0], gt[3], dx, dy], np.float64),
           "geographic": np.array(geographic), "libc": np.array(M.libc_tag())}
    agree = []
    with tempfile.TemporaryDirectory() as d:
        f = lambda s: os.path.join(d, s)  # noqa: E731
        T.write_raster(f("ang.tif"), ang, M.ANG_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("fel.tif"), fel, M.FEL_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("wg.tif"), wg, M.WG_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("rc.tif"), rc, M.RC_NODATA, geotransform=gt, geographic=geographic)
        T.write_raster(f("ass.tif"), ass, M.ASS_NODATA, geotransform=gt, geographic=geographic)

        def same(a, b):
            return bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
        rl = ["-ang", f("ang.tif"), "-wg", f("wg.tif"), "-rc", f("rc.tif")]
        O.run_ref(exes["retlimflow"], rl + ["-qrl", f("qrl.tif")])
        res["qrl"], _ = T.read_raster(f("qrl.tif"))
        if check_ranks:
            O.run_ref(exes["retlimflow"], rl + ["-qrl", f("qrl3.tif")], check_ranks)
            agree.append(("qrl", same(T.read_raster(f("qrl3.tif"))[0], res["qrl"])))
        av = ["-ang", f("ang.tif"), "-fel", f("fel.tif"), "-ass", f("ass.tif")]
        for sfx, direct, (thresh, alpha) in M.variants():
            extra = ["-thresh", str(thresh), "-alpha", str(alpha)] + (["-direct"] if direct else [])
            O.run_ref(exes["dinfavalanche"], av + ["-rz", f(f"rz{sfx}.tif"), "-dfs", f(f"dfs{sfx}.tif")] + extra)
            res["rz" + sfx], _ = T.read_raster(f(f"rz{sfx}.tif"))
            res["dfs" + sfx], _ = T.read_raster(f(f"dfs{sfx}.tif"))
            if check_ranks:
                O.run_ref(exes["dinfavalanche"], av + ["-rz", f(f"rz3{sfx}.tif"), "-dfs", f(f"dfs3{sfx}.tif")] + extra, check_ranks)
                agree.append(("rz" + sfx, same(T.read_raster(f(f"rz3{sfx}.tif"))[0], res["rz" + sfx])))
                agree.append(("dfs" + sfx, same(T.read_raster(f(f"dfs3{sfx}.tif"))[0], res["dfs" + sfx])))
    np.savez_compressed(os.path.join(OUT, f"aval_{name}.npz"), **res)
    q = res["qrl"]
    print(name, ang.shape, "qrl max", float(q[q > -1e30].max()), "qrl nodata", int((q < -1e30).sum()), "clamped", int((q == 0).sum()),
          "file bytes", os.path.getsize(os.path.join(OUT, f"aval_{name}.npz")))
    # the restatement alone: agreement and the tainted share
    gg = M.load_golden(name)
    print("  source seed", seed, "sources", int((ass > 0).sum()))
    print("  restatement qrl:", "same" if same(R.retlimflow(ang, wg, rc, dxc=g["dxc"], dyc=g["dyc"]), q) else "DIFFERENT")
    for sfx, direct, ta in M.variants():
        rz, dfs, taint = M.run_aval(R, gg, direct, ta)
        has = res["rz" + sfx] > -1e30
        share = taint.sum() / max(has.sum(), 1)
        print(f"  {sfx[1:]:9s} cells with rz {int(has.sum()):6d}  tainted {int(taint.sum()):4d} ({share:.4f})  restatement rz {'same' if same(rz, res['rz' + sfx]) else 'DIFFERENT'}"
              f"  dfs {'same' if same(dfs, res['dfs' + sfx]) else 'DIFFERENT'}")
        assert share <= M.MAX_TAINT_SHARE, "too many tainted cells: choose other sources"
    if agree:
        print(f"  {check_ranks} ranks vs 1 rank:", "; ".join(f"{k}: {'same' if a else 'DIFFERENT'}" for k, a in agree))
        assert all(a for _, a in agree), "the reference's multi-rank run differs from its 1-rank run"


if __name__ == "__main__":
    O.build()
    with tempfile.TemporaryDirectory() as tmp:
        exes = {"retlimflow": build_tool(tmp, ("RetlimFlow", "RetLimFlowmn"), "retlimflow"),
                "dinfavalanche": build_tool(tmp, ("DinfAvalanche", "DinfAvalanchemn"), "dinfavalanche")}
        R = M.compile(tmp)
        for c in CASES:
            make(exes, R, c, check_ranks=3 if c in ("holes", "plain", "rect_dxdy") else 0)
