"""CatchHydroGeo and InunDepth on one MI355X, HBM-resident synthetic inputs (generated on the device: a gamma-like HAND raster with 1 % zeros,
slopes in [0, 0.8), Voronoi catchments grown from a coarse seed grid; no file of the reference is read).  One JSON line: ms (library-side
HIP-event time of the call), Mcells/s, achieved GB/s against 12 B/cell (CatchHydroGeo: hand + catch + slp; InunDepth map: hand + catch + map; 14 with
the 2-byte mask), the slab bytes, the (tile, catchment) records, records per tile and the most records of one tile.  The keyed reduction has no separate slow
path: `max_records_in_a_tile` and `records_per_tile` say how often its per-index loop ran.
usage: python scripts/bench_hand.py [--size 16384] [--stages 83] [--catchments 4000]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import taudem_amd as T

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=16384)
ap.add_argument("--stages", type=int, default=83)
ap.add_argument("--catchments", type=int, default=4000)
a = ap.parse_args()
n, dev = a.size, "cuda:0"
ctx = T.Context(0)
g = torch.Generator(device=dev).manual_seed(11)
hand = (-3.0 * torch.log(torch.rand((n, n), device=dev, generator=g).clamp_min(1e-6))).to(torch.float32)
hand[torch.rand((n, n), device=dev, generator=g) < 0.01] = 0.0
slp = (0.8 * torch.rand((n, n), device=dev, generator=g)).to(torch.float32)
# Voronoi-like catchments: a k x k grid of seeds, every cell takes the label of the jittered seed of its coarse block (borders wander with the jitter)
k = max(1, int(round(a.catchments ** 0.5)))
yy = torch.arange(n, device=dev, dtype=torch.float32)[:, None].expand(n, n)
xx = torch.arange(n, device=dev, dtype=torch.float32)[None, :].expand(n, n)
cell = n / k
jy = (torch.sin(xx * 0.013) * 0.3 * cell)
jx = (torch.cos(yy * 0.011) * 0.3 * cell)
lab = (((yy + jy) / cell).floor().clamp(0, k - 1) * k + ((xx + jx) / cell).floor().clamp(0, k - 1)).to(torch.int32) + 1
del yy, xx, jy, jx
ids = np.arange(1, k * k + 1, dtype=np.int32)
stages = np.linspace(0.0, 25.0, a.stages)
res = {"size": n, "stages": a.stages, "catchments": int(ids.size)}

def timed(fn):
    fn()                       # warm-up (scratch allocation)
    torch.cuda.synchronize()
    return fn()

out = timed(lambda: ctx.catchhydrogeo(hand, lab, slp, ids, stages, dx=10.0, dy=10.0, stats=True))
st = out[-1]
tiles = ((n + 63) // 64) ** 2
res["catchhydrogeo"] = {"ms": st["ms_total"], "mcells_per_s": n * n / st["ms_total"] / 1e3, "gb_per_s_12B": 12.0 * n * n / st["ms_total"] / 1e6,
                        "slab_bytes": st["flats_initial"], "records": st["cells_evaluated"], "records_per_tile": st["cells_evaluated"] / tiles,
                        "max_records_in_a_tile": st["levels_fall_max"], "stage_chunks": st["rounds"], "ms_count": st["ms_misc"], "ms_tiles_and_reduce": st["ms_accum"]}
depth = np.full(ids.size, 3.0, np.float32)
for name, mask, b in (("inundepth_map", None, 12.0), ("inundepth_map_mask", torch.zeros((n, n), device=dev, dtype=torch.int16), 14.0)):
    out = timed(lambda: ctx.inundepth(hand, lab, ids, depth, mask=mask, area=False, stats=True))
    ms = out[-1]["ms_stencil"] or out[-1]["ms_total"]
    res[name] = {"ms": ms, "ms_call": out[-1]["ms_total"], "mcells_per_s": n * n / ms / 1e3, f"gb_per_s_{int(b)}B": b * n * n / ms / 1e6}
out = timed(lambda: ctx.inundepth(hand, lab, ids, depth, area=True, dx=10.0, dy=10.0, stats=True))
res["inundepth_with_area"] = {"ms": out[-1]["ms_total"], "mcells_per_s": n * n / out[-1]["ms_total"] / 1e3}
print(json.dumps(res))
