"""The SINMAP parameter region grid on one MI355X.  Two polygon inputs on an n x n raster of 30 m cells:
  (a) watersheds  the watershed polygons of the product's own pipeline on a synthetic fractal DEM (the input of bench_polygonize.py: pitremove,
                  d8flowdir, aread8, src = ad8 >= the threshold that leaves about 1 % of the cells on streams, streamnet, polygonize), burned back by
                  their ids + 1 (0 is nodata): many small features, short edges; the result is checked against w + 1
  (b) voronoi     the Voronoi cells of twelve seeded points clipped to the raster: few features that span it, long straight edges
and the resample mode from a source grid of n/4 x n/4 cells of 120 m, offset by a fraction of a cell.
Method: a warm-up call, then --steps timed calls.  Per call the library's own phase clocks (prepare, cross, fill, write: wall time, each phase ended
with the stream drained) and the device events around the launches of each kernel class (cross: the memset of the bitmaps and the crossing kernel;
fill; misc: the uploads, the memset of the winner words, the streaming pass and its read-back).  The yardstick is a device copy of the int16 output
(n * n * 2 bytes read and as many written), timed by device events in the same run.  Writes one JSON file.
usage: python scripts/bench_regiongrid.py [--size 16384] [--steps 3] [--warmup 1] [--share 0.01] [--out profiles/regiongrid_bench_<size>.json]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import taudem_amd as T

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=16384)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--share", type=float, default=0.01)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n = a.size
out_path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", f"regiongrid_bench_{n}.json")
GT = (4.1e5, 30.0, 0.0, 4.6e6, 0.0, -30.0)
ND = -2147483647
ctx = T.Context(0)


def spread(v):
    v = np.asarray(v, np.float64)
    return {"mean_ms": float(v.mean()), "min_ms": float(v.min()), "max_ms": float(v.max())}


def watersheds():
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
    del ordg, p, src, fel, ad8, tree, coord, sample
    with ctx.polygonize(w) as pg:
        packed, ids = pg.packed(GT), pg.ids.copy()
    ctx.release_scratch()
    torch.cuda.empty_cache()
    ids = ids.astype(np.int64) + 1          # StreamNet numbers its watersheds from 0, and 0 is the region grid's nodata: burn id + 1
    assert ids.min() >= 1 and ids.max() <= 32767, "the watershed ids of this input, plus one, fit the region grid"
    want = torch.where(w == ND, torch.zeros_like(w), w + 1).to(torch.int16)
    del w
    return packed, ids, want


def voronoi():
    """The cell of seed i: the raster's rectangle cut by the half-plane nearer to i than to j, for every other seed j (Sutherland-Hodgman)."""
    rng = np.random.default_rng(12)
    pts = rng.uniform(0.05, 0.95, (12, 2)) * n
    cells = []
    for i in range(12):
        poly = [(0.0, 0.0), (float(n), 0.0), (float(n), float(n)), (0.0, float(n))]
        for j in range(12):
            if j == i or not poly:
                continue
            nrm, mid = pts[j] - pts[i], (pts[i] + pts[j]) / 2
            side = lambda q: float(np.dot(np.asarray(q) - mid, nrm))   # noqa: E731  <= 0: nearer to i
            nxt = []
            for k in range(len(poly)):
                p0, p1 = poly[k], poly[(k + 1) % len(poly)]
                s0, s1 = side(p0), side(p1)
                if s0 <= 0:
                    nxt.append(p0)
                if (s0 <= 0) != (s1 <= 0):
                    t = s0 / (s0 - s1)
                    nxt.append((p0[0] + t * (p1[0] - p0[0]), p0[1] + t * (p1[1] - p0[1])))
            poly = nxt
        cells.append([[(GT[0] + x * GT[1], GT[3] + y * GT[5]) for x, y in poly]])
    return cells, list(range(1, 13))


out = torch.empty((n, n), dtype=torch.int16, device="cuda:0")
out.fill_(1)
dst = torch.empty_like(out)
copy_ms = []
for i in range(12):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); dst.copy_(out); e1.record(); torch.cuda.synchronize()
    if i >= 2:
        copy_ms.append(e0.elapsed_time(e1))
del dst
copy_med = float(np.median(copy_ms))
copy_gbs = 2 * n * n * 2 / (copy_med * 1e-3) / 1e9


def measure(name, **kw):
    calls, phases, events, ws, ids = [], [], [], 0, None
    for i in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, ids, st = ctx.regiongrid((n, n), GT, out=out, stats=True, **kw)
        t1 = time.perf_counter()
        print(f"{name} call {i}: {(t1 - t0) * 1e3:.1f} ms, phases {st['phases']}, device events: cross {st['ms_accum']:.3f} fill {st['ms_stencil']:.3f} "
              f"misc {st['ms_misc']:.3f} ms, workspace {st['workspace_bytes']} bytes", flush=True)
        if i >= a.warmup:
            calls.append((t1 - t0) * 1e3); phases.append(st["phases"]); events.append((st["ms_accum"], st["ms_stencil"], st["ms_misc"])); ws = st["workspace_bytes"]
    plain = []          # the same call without the phase clocks: nothing drains the stream between the kernels
    for i in range(a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.regiongrid((n, n), GT, out=out, **kw)
        plain.append((time.perf_counter() - t0) * 1e3)
    ev = {k: spread([e[j] for e in events]) for j, k in enumerate(("cross", "fill", "misc"))}
    device_ms = sum(v["mean_ms"] for v in ev.values())
    return {"ids": int(ids.size), "call_wall": spread(calls), "call_wall_without_phase_clocks": spread(plain), "phases_wall": {k: spread([p[k] for p in phases]) for k in phases[0]}, "device_events": ev,
            "device_ms": device_ms, "device_over_copy_of_the_output": device_ms / copy_med, "workspace_bytes": ws,
            "launches": {"cross": int(st["launches_accum"]), "fill": int(st["launches_stencil"]), "misc": int(st["launches_misc"])}}


res = {"size": n, "cells": n * n, "steps": a.steps, "warmup": a.warmup, "geotransform": GT,
       "device_copy_of_the_output": {**spread(copy_ms), "median_ms": copy_med, "gb_per_s_read_plus_written": copy_gbs}}

packed, ids, want = watersheds()
print(f"watersheds ready: {len(packed)} features, {packed.x.size} vertices", flush=True)
res["watersheds"] = {"features": len(packed), "rings": int(packed.ring_first.size - 1), "vertices": int(packed.x.size), "stream_share": a.share,
                     **measure("watersheds", polygons=packed, values=ids)}
res["watersheds"]["equals_w"] = bool(torch.equal(out, want))
assert res["watersheds"]["equals_w"], "the region grid of the watershed polygons is the watershed grid"
del packed, want

cells, values = voronoi()
res["voronoi"] = {"features": 12, "vertices": int(sum(len(c[0]) for c in cells)), **measure("voronoi", polygons=cells, values=values)}
res["voronoi"]["cells_without_a_region"] = int((out == 0).sum())

m = max(n // 4, 1)
src = torch.from_numpy(np.random.default_rng(3).integers(1, 13, (m, m)).astype(np.int32)).to("cuda:0")
sgt = (GT[0] - 47.3, 120.0, 0.0, GT[3] + 33.7, 0.0, -120.0)
res["resample"] = {"source_cells": m * m, "source_geotransform": sgt, **measure("resample", source=src, source_gt=sgt, source_nodata=-9)}

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
