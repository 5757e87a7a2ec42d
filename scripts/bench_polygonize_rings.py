"""The two ring builders of the watershed polygons on one MI355X, alternating in one run: rings="host" (the default: the edge columns come down, one
host core walks them) and rings="device" (polygon_rings_device.hip: only the finished layer comes down).  Inputs: the watershed grid w of the product's own
pipeline on a synthetic fractal DEM with about 1 % stream cells (the input of scripts/bench_polygonize.py), HBM-resident; or --checker: a checkerboard
of two ids, four edges and one ring per cell, the many-rings regime.  Writes one JSON file: for either path the phases of the call and its wall time; for
the device path the sub-phases, the jump rounds, the workspace and the bytes of the result; a device copy of as many bytes as the edge columns hold
(20 per edge) as the yardstick of the ring phase; whether the two paths gave the same arrays.
usage: python scripts/bench_polygonize_rings.py [--size 16384 | --checker 2048] [--steps 2 (5 below 8192^2)] [--warmup 1] [--share 0.01] [--out FILE]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import taudem_amd as T

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=16384)
ap.add_argument("--checker", type=int, default=0)
ap.add_argument("--steps", type=int, default=None)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--share", type=float, default=0.01)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n = a.checker or a.size
if a.steps is None:
    a.steps = 2 if n >= 8192 else 5
tag = f"checker{n}" if a.checker else str(n)
out_path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", f"polygonize_rings_bench_{tag}.json")
ctx = T.Context(0)
if a.checker:
    i = torch.arange(n, device="cuda:0", dtype=torch.int32)
    w = (1 + (i[:, None] + i[None, :]) % 2).to(torch.int32).contiguous()
    del i
else:
    dem = ctx.synth_dem(n, seed=1234)
    fel = ctx.pitremove(dem, -9999.0)
    del dem
    p, sd8 = ctx.d8flowdir(fel, -3.0e38, 30.0, 30.0)
    del sd8
    ad8 = ctx.aread8(p, -32768, contcheck=False)
    sample = ad8.flatten()[:: max(1, n * n // 4_000_000)]
    thresh = float(torch.sort(sample).values[int((1.0 - a.share) * (sample.numel() - 1))])
    src = (ad8 >= thresh).to(torch.int32)
    del sample
    ordg, w, tree, coord = ctx.streamnet(p, src, fel, ad8, dx=30.0, dy=30.0)
    del ordg, p, src, fel, ad8, tree, coord
    ctx.release_scratch()
torch.cuda.empty_cache()
print(f"w ready: {n} x {n} ({tag})", flush=True)


def spread(v):
    v = np.asarray(v, np.float64)
    return {"mean_ms": float(v.mean()), "min_ms": float(v.min()), "max_ms": float(v.max())}


ARRAYS = ("ids", "cells", "poly_first", "ring_first", "vert_first", "vertices")
runs = {"host": [], "device": []}
shape, kept, same = None, {}, True
for i in range(a.warmup + a.steps):
    for rings in ("host", "device"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pg = ctx.polygonize_rings(w, rings=rings)
        with pg:
            t1 = time.perf_counter()
            rec = {"call_ms": (t1 - t0) * 1e3, "phases": pg.phases, "ring_phases": pg.ring_phases, "rounds": pg.ring_rounds, "workspace_bytes": pg.ring_workspace_bytes}
            shape = {"edges": pg.edges, "features": int(pg.ids.size), "polygons": int(pg.ring_first.size - 1), "rings": int(pg.vert_first.size - 1),
                     "vertices": int(pg.vertices.shape[0]), "result_bytes": int(sum(getattr(pg, k).nbytes for k in ARRAYS))}
            if i == 0:   # the two paths' arrays, compared once
                kept[rings] = [getattr(pg, k).copy() for k in ARRAYS]
        print(f"call {i} {rings}: {rec['call_ms']:.1f} ms, phases {rec['phases']}, ring phases {rec['ring_phases']}, rounds {rec['rounds']}", flush=True)
        if i >= a.warmup:
            runs[rings].append(rec)
    if i == 0:
        same = all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(kept["host"], kept["device"]))
        kept = {}
assert same, "the two ring builders must give the same arrays"

# the yardstick of the ring phase: a device copy of as many bytes as the edge columns hold
nbytes = max(shape["edges"] * 20, 1 << 20)
srcb = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0").zero_()
dstb = torch.empty_like(srcb)
copy_ms = []
for i in range(12):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); dstb.copy_(srcb); e1.record(); torch.cuda.synchronize()
    if i >= 2:
        copy_ms.append(e0.elapsed_time(e1))
del srcb, dstb
copy = float(np.median(copy_ms))


def path(recs):
    out = {"call_wall": spread([r["call_ms"] for r in recs]), "phases": {k: spread([r["phases"][k] for r in recs]) for k in recs[0]["phases"]},
           "phases_total_ms": float(np.mean([sum(r["phases"].values()) for r in recs]))}
    if recs[0]["ring_phases"]:
        out["ring_phases"] = {k: spread([r["ring_phases"][k] for r in recs]) for k in recs[0]["ring_phases"]}
        out["rounds"], out["workspace_bytes"] = recs[0]["rounds"], recs[0]["workspace_bytes"]
    return out


host, dev = path(runs["host"]), path(runs["device"])
res = {"input": tag, "size": n, "cells": n * n, "steps": a.steps, "warmup": a.warmup, **shape, "edge_column_bytes": shape["edges"] * 20,
       "same_arrays": bool(same), "host": host, "device": dev,
       "device_copy_of_the_edge_columns_bytes": {**spread(copy_ms), "median_ms": copy, "bytes": nbytes},
       "device_ring_phase_over_that_copy": dev["phases"]["rings"]["mean_ms"] / copy,
       "ring_phase_host_over_device": host["phases"]["rings"]["mean_ms"] / dev["phases"]["rings"]["mean_ms"],
       "call_host_over_device": host["call_wall"]["mean_ms"] / dev["call_wall"]["mean_ms"]}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
