"""ConnectDown and MoveOutletsToStrm on one MI355X, HBM-resident: p and ad8 of a synthetic fractal DEM come from the product, src = ad8 >= the
threshold that leaves about 1 % of the cells on streams, w is StreamNet's watershed grid of them.  Writes one JSON file with, after a warm-up and over
a window of about a second (mean and spread):
  * the device time (HIP events around the launches) of ConnectDown's phases: the max-id reduction over w, the arg-max pass over w and ad8, the decode
    of the table, the walk; and the pass's bytes per second taken as 8 B x cells over its time, with its share of the HBM peak;
  * in the same run, alternating with it, a device-to-device copy of the w and ad8 arrays (device events): it moves twice the bytes the pass reads
    and is the pass's yardstick - the pass should take no longer;
  * the run-length statistics of w in row-major order (what decides how many atomics the pass issues);
  * the walk of 1 000 outlets (MoveOutletsToStrm, -md 50) and the whole calls (host clock around calls that end in a synchronise);
  * the arg-max pass on checkerboard ids (one atomic per cell): the time only.
The reference's two tools are not built where this runs: "not measured".
usage: python scripts/bench_outlets.py [--size 16384] [--window 1.0] [--warmup 3] [--share 0.01] [--out profiles/outlets_bench_<size>.json]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import taudem_amd as T

HBM_PEAK_TBS = 8.0   # HBM3E peak of the MI355X, spec

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=16384)
ap.add_argument("--window", type=float, default=1.0, help="seconds of timed ConnectDown calls")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--share", type=float, default=0.01)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n = a.size
out_path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", f"outlets_bench_{n}.json")
ctx = T.Context(0)
dem = ctx.synth_dem(n, seed=1234)
fel = ctx.pitremove(dem, -9999.0)
del dem
p, sd8 = ctx.d8flowdir(fel, -3.0e38, 30.0, 30.0)
del sd8
ad8 = ctx.aread8(p, -32768, contcheck=False)
sample = ad8.flatten()[:: max(1, n * n // 4_000_000)]
thresh = float(torch.sort(sample).values[int((1.0 - a.share) * (sample.numel() - 1))])
src = (ad8 >= thresh).to(torch.int32)
ordg, w, tree, coord = ctx.streamnet(p, src, fel, ad8, dx=30.0, dy=30.0)
del ordg, fel, sample
ctx.release_scratch()
flat = w.flatten()
heads = int((flat[1:] != flat[:-1]).sum()) + 1
labelled = int((flat != -2147483647).sum())
runs = {"runs_row_major": heads, "mean_run_cells": n * n / heads, "labelled_share": labelled / (n * n), "watersheds": int(tree.shape[0])}
del flat
# 1 000 outlets spread over the raster
rng = np.random.default_rng(7)
outlets = (rng.integers(0, n, 1000).astype(np.int32), rng.integers(0, n, 1000).astype(np.int32))
w2, ad82 = torch.empty_like(w), torch.empty_like(ad8)
yy = torch.arange(n, device=w.device, dtype=torch.int32)
w_cb = ((yy[:, None] + yy[None, :]) % 2 + 1).contiguous()
del yy


def spread(v):
    v = np.asarray(v, np.float64)
    return {"mean_ms": float(v.mean()), "min_ms": float(v.min()), "max_ms": float(v.max()), "samples": int(v.size)}


def copy_ms():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    w2.copy_(w); ad82.copy_(ad8)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


phases, copies, calls, walk_dev, walk_calls, cb = [], [], [], [], [], []
points = 0
i, timed = 0, 0.0
while i < a.warmup or timed < a.window:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ctx.connectdown(p, w, ad8, 10, phases=True)
    t1 = time.perf_counter()
    c = copy_ms()
    t2 = time.perf_counter()
    rx, ry, rd, st = ctx.moveoutletstostrm(p, src, outlets, 50, src_nodata=-2147483647, stats=True)
    t3 = time.perf_counter()
    if i >= a.warmup:
        phases.append(res[7]); copies.append(c); calls.append((t1 - t0) * 1e3); walk_dev.append(st["ms_accum"]); walk_calls.append((t3 - t2) * 1e3)
        timed += t1 - t0
    points = int(res[0].size)
    i += 1
for _ in range(a.warmup + 5):
    cb.append(ctx.connectdown(p, w_cb, ad8, 0, phases=True)[7]["argmax"])
cb = cb[a.warmup:]
argmax_ms = float(np.mean([m["argmax"] for m in phases]))
copy_mean = float(np.mean(copies))
res = {"size": n, "cells": n * n, "threshold": thresh, "points": points, "outlets": 1000, "moved": int((rd >= 0).sum()), "warmup": a.warmup, "window_s": timed,
       "w_runs": runs,
       "connectdown_phases_device": {k: spread([m[k] for m in phases]) for k in phases[0]},
       "argmax_with_maxid_ms": float(np.mean([m["argmax"] + m["maxid"] for m in phases])),
       "argmax_bytes_per_s": 8.0 * n * n / (argmax_ms * 1e-3),
       "argmax_share_of_hbm_peak": 8.0 * n * n / (argmax_ms * 1e-3) / (HBM_PEAK_TBS * 1e12), "hbm_peak_tb_s_spec": HBM_PEAK_TBS,
       "yardstick_copy_of_w_and_ad8_device": spread(copies), "copy_bytes_per_s": 16.0 * n * n / (copy_mean * 1e-3),
       "argmax_over_copy": argmax_ms / copy_mean, "meets_the_bar": bool(argmax_ms <= copy_mean),
       "connectdown_call_wall": spread(calls),
       "moveoutlets_walk_device": spread(walk_dev), "moveoutlets_call_wall": spread(walk_calls),
       "checkerboard_argmax_device": spread(cb),
       "reference_tools_on_host_cores": "not measured"}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
