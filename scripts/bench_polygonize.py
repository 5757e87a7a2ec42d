"""Watershed polygons on one MI355X: the watershed grid w comes from the product's own pipeline on a synthetic fractal DEM (pitremove, d8flowdir, aread8,
src = ad8 >= the threshold that leaves about 1 % of the cells on streams, streamnet), HBM-resident.  Writes one JSON file with the edges per cell, the wall
time of each phase of Context.polygonize (count, scan, emit, download, rings: tdx_polygonize's own clocks, each phase ended with the stream drained; mean
and spread over the timed steps after a warm-up), the two device passes (count + emit, timed by device events) against a device copy: the passes read w twice and write the three
edge columns, and a torch copy of w gives the rate at which this device moves bytes (read + written) in the same run; and the host's share of the call.
usage: python scripts/bench_polygonize.py [--size 16384] [--steps 2 (5 below 8192^2)] [--warmup 1] [--share 0.01] [--out profiles/polygonize_bench_<size>.json]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import taudem_amd as T

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=16384)
ap.add_argument("--steps", type=int, default=None)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--share", type=float, default=0.01)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n = a.size
if a.steps is None:
    a.steps = 2 if n >= 8192 else 5
out_path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", f"polygonize_bench_{n}.json")
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
del sample
ordg, w, tree, coord = ctx.streamnet(p, src, fel, ad8, dx=30.0, dy=30.0)
del ordg, p, src, fel, ad8, tree, coord
ctx.release_scratch()
torch.cuda.empty_cache()
ids_present = int((w != -2147483647).sum())
print(f"w ready: {n} x {n}, {ids_present} cells with an id", flush=True)


def spread(v):
    v = np.asarray(v, np.float64)
    return {"mean_ms": float(v.mean()), "min_ms": float(v.min()), "max_ms": float(v.max())}


# the yardstick: a device copy of w, n * n * 4 bytes read and as many written
dst = torch.empty_like(w)
copy_ms = []
for i in range(12):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); dst.copy_(w); e1.record(); torch.cuda.synchronize()
    if i >= 2:
        copy_ms.append(e0.elapsed_time(e1))
del dst
copy_gbs = 2 * n * n * 4 / (np.median(copy_ms) * 1e-3) / 1e9

phases, calls, events, shape = [], [], [], None
for i in range(a.warmup + a.steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pg, st = ctx.polygonize(w, stats=True)
    with pg:
        t1 = time.perf_counter()
        shape = {"edges": pg.edges, "features": int(pg.ids.size), "polygons": int(pg.ring_first.size - 1), "rings": int(pg.vert_first.size - 1),
                 "vertices": int(pg.vertices.shape[0]), "cells_in_features": int(pg.cells.sum())}
        ms = pg.phases
    print(f"call {i}: {(t1 - t0) * 1e3:.1f} ms, phases {ms}, device events: passes {st['ms_stencil']:.3f} ms, scan + download {st['ms_misc']:.3f} ms", flush=True)
    if i >= a.warmup:
        phases.append(ms); calls.append((t1 - t0) * 1e3); events.append((st["ms_stencil"], st["ms_misc"]))
assert shape["cells_in_features"] == ids_present, "cells is a self-check: it must equal the count of cells with an id"
mean = {k: float(np.mean([m[k] for m in phases])) for k in phases[0]}
pass_bytes = 2 * n * n * 4 + shape["edges"] * 20
passes_ms = float(np.mean([e[0] for e in events]))   # device events around the two passes: a phase clock also holds what the host waits for after it sat idle
total_ms = sum(mean.values())
res = {"size": n, "cells": n * n, "threshold": thresh, "stream_share": a.share, "steps": a.steps, "warmup": a.warmup, **shape,
       "edges_per_cell": shape["edges"] / (n * n),
       "phases": {k: spread([m[k] for m in phases]) for k in phases[0]},
       "call_wall": spread(calls),   # the Python call: the phases plus the copy of the polygon arrays
       "device_copy_of_w": {**spread(copy_ms), "gb_per_s_read_plus_written": copy_gbs},
       "device_events": {"passes": spread([e[0] for e in events]), "scan_and_download": spread([e[1] for e in events])},
       "device_passes": {"ms": passes_ms, "bytes": pass_bytes, "gb_per_s": pass_bytes / (passes_ms * 1e-3) / 1e9,
                         "copy_of_the_same_bytes_ms": pass_bytes / (copy_gbs * 1e9) * 1e3, "over_copy_of_the_same_bytes": passes_ms / (pass_bytes / (copy_gbs * 1e9) * 1e3),
                         "over_one_copy_of_w": passes_ms / float(np.median(copy_ms))},
       "host_rings_share_of_phases": mean["rings"] / total_ms, "download_share_of_phases": mean["download"] / total_ms}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
