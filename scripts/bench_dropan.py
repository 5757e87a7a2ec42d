"""DropAnalysis on one MI355X, HBM-resident inputs: a synthetic DEM (Context.synth_dem) through the project's own pitremove / d8flowdir / aread8, ssa = ad8,
outlets on the largest-area cells.  One JSON line: ms of the whole call (library-side HIP-event time), ms per threshold, ms of the sweeps and of the
set-up / statistics passes, rounds, Mcells/s per threshold (cells x nthresh / time: the reference's own banner estimates 2e-7 x cells x nthresh minutes)
and the table's optimum.  No file of the reference is read.
usage: python scripts/bench_dropan.py [--size 8192] [--nthresh 10] [--min 5] [--max 5000] [--steptype 0]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import taudem_amd as T

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=8192)
ap.add_argument("--nthresh", type=int, default=10)
ap.add_argument("--min", type=float, default=5.0)
ap.add_argument("--max", type=float, default=5000.0)
ap.add_argument("--steptype", type=int, default=0)
a = ap.parse_args()
n = a.size
ctx = T.Context(0)
dem = ctx.synth_dem(n, seed=7)
fel = ctx.pitremove(dem, -9999.0)
p, _ = ctx.d8flowdir(fel, float(T.FEL_NODATA), 30.0, 30.0)
ad8 = ctx.aread8(p, contcheck=False)
del dem
flat = torch.where((p >= 1) & (p <= 8), ad8, torch.full_like(ad8, -2.0)).reshape(-1)
idx = torch.topk(flat, 8).indices.cpu().numpy()
outlets = ((idx % n).astype(np.int32), (idx // n).astype(np.int32))

def run():
    return ctx.dropanalysis(ad8, p, fel, ad8, outlets, thresh_min=a.min, thresh_max=a.max, nthresh=a.nthresh, steptype=a.steptype, dx=30.0, dy=30.0, stats=True)

run()                          # warm-up (scratch allocation)
torch.cuda.synchronize()
out = run()
st = out[-1]
print(json.dumps({"size": n, "nthresh": a.nthresh, "ms": st["ms_total"], "ms_per_threshold": st["ms_total"] / a.nthresh, "ms_sweeps": st["ms_accum"],
                  "ms_setup": st["ms_stencil"], "ms_statistics": st["ms_misc"], "rounds": st["cells_evaluated"],
                  "mcells_per_s_per_threshold": n * n * a.nthresh / st["ms_total"] / 1e3, "n1": out[1].tolist(), "n2": out[2].tolist(),
                  "optimum": None if out[7] is None else float(out[7])}))
