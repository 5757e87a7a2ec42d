"""StreamNet on one MI355X, HBM-resident: fel, p and ad8 of a synthetic fractal DEM come from the product, src = ad8 >= the threshold that leaves about
1 % of the cells on streams (the share is printed).  Writes one JSON file with the wall time of each phase of the call (set-up, length sweep,
compaction, host link build, scatter, label sweep, total: tdx_streamnet's own clocks, each phase ended with the stream drained; mean and spread over the
timed steps after a warm-up) and, from the same run, the times of d8hdisttostrm (same src) and gagewatershed (gauges on the largest stream ends) on the
same p: the two new sweeps use their engine, so these are the yardstick.
--links both: the two link builders instead, alternating in one process on the same HBM-resident inputs (host, device, host, device, ...: one warm-up
pair, then timed pairs): for either the phases and the wall time of the call, for the device builder its sub-phases, round counts, workspace and the
bytes of coord that come down; ord, w, tree and coord of the two are compared once, and no record is written if they differ.  That record goes to
profiles/streamnet_links_bench_<size>.json.
usage: python scripts/bench_streamnet.py [--size 16384] [--steps 3 (40 below 8192^2)] [--warmup 1] [--share 0.01] [--links host|both] [--out FILE]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import taudem_amd as T

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=16384)
ap.add_argument("--steps", type=int, default=None, help="timed steps (default: 3 from 8192^2 up, 40 below, so that the timed window is about a second)")
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--share", type=float, default=0.01)
ap.add_argument("--links", default="host", choices=("host", "both"))
ap.add_argument("--out", default=None)
a = ap.parse_args()
n = a.size
if a.steps is None:
    a.steps = 3 if n >= 8192 else 40
out_path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                 f"streamnet_links_bench_{n}.json" if a.links == "both" else f"streamnet_bench_{n}.json")
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
stream = (src > 0) & (p != -32768)
share = float(stream.sum()) / (n * n)
# gauges of the yardstick: the 32 largest-area stream cells
top = torch.topk(torch.where(stream, ad8, torch.zeros_like(ad8)).flatten(), 32).indices.cpu().numpy()
gauges = ((top % n).astype(np.int32), (top // n).astype(np.int32), np.arange(1, 33, dtype=np.int32))
del stream, sample


def spread(v):
    v = np.asarray(v, np.float64)
    return {"mean_ms": float(v.mean()), "min_ms": float(v.min()), "max_ms": float(v.max())}


def write(res):
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if a.links == "both":
    runs, kept, same, shape = {"host": [], "device": []}, {}, True, {}
    for i in range(a.warmup + a.steps):
        for where in ("host", "device"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ordg, w, tree, coord, ms = ctx.streamnet(p, src, fel, ad8, dx=30.0, dy=30.0, phases=True, links=where)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            sub = ms.pop("links_device", None)
            rec = {"call_ms": (t1 - t0) * 1e3, "phases": ms, "links_device": sub}
            shape = {"links": int(tree.shape[0]), "points": int(coord.shape[0]), "tree_bytes": int(tree.nbytes), "coord_bytes": int(coord.nbytes)}
            if i == 0:   # the two builders' outputs, compared once
                kept[where] = (ordg.cpu().numpy(), w.cpu().numpy(), tree, coord.view(np.uint64))
            print(f"call {i} {where}: {rec['call_ms']:.1f} ms, phases {ms}, device builder {sub}", flush=True)
            if i >= a.warmup:
                runs[where].append(rec)
            del ordg, w, tree, coord
        if i == 0:
            same = all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(kept["host"], kept["device"]))
            kept = {}
            if not same:
                sys.exit("the two link builders gave different ord, w, tree or coord: no record written")

    def path(recs):
        out = {"call_wall": spread([r["call_ms"] for r in recs]), "phases": {k: spread([r["phases"][k] for r in recs]) for k in recs[0]["phases"]}}
        sub = recs[0]["links_device"]
        if sub:
            out["links_device"] = {k: spread([r["links_device"][k] for r in recs]) for k in T._lib.STREAMNET_LINK_PHASES}
            out.update(jump_rounds=sub["jump_rounds"], level_rounds=sub["level_rounds"], workspace_bytes=sub["workspace_bytes"])
        return out

    host, dev = path(runs["host"]), path(runs["device"])
    write({"size": n, "cells": n * n, "threshold": thresh, "stream_share": share, "stream_cells": int(round(share * n * n)), **shape, "steps": a.steps, "warmup": a.warmup,
           "order": "host, device alternating in one process", "same_ord_w_tree_coord": bool(same), "host": host, "device": dev,
           "link_phase_host_over_device": host["phases"]["links"]["mean_ms"] / dev["phases"]["links"]["mean_ms"],
           "call_host_over_device": host["call_wall"]["mean_ms"] / dev["call_wall"]["mean_ms"]})
    sys.exit(0)

phases, calls, dist_ms, gage_ms, links = [], [], [], [], 0
for i in range(a.warmup + a.steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ordg, w, tree, coord, ms = ctx.streamnet(p, src, fel, ad8, dx=30.0, dy=30.0, phases=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    _, sd = ctx.d8hdisttostrm(p, src, 1, dx=30.0, dy=30.0, src_nodata=-2147483647, stats=True)
    _, _, sg = ctx.gagewatershed(p, gauges, stats=True)
    if i >= a.warmup:
        phases.append(ms); calls.append((t1 - t0) * 1e3); dist_ms.append(sd["ms_total"]); gage_ms.append(sg["ms_total"])
    links = int(tree.shape[0])
    del ordg, w
res = {"size": n, "cells": n * n, "threshold": thresh, "stream_share": share, "stream_cells": int(round(share * n * n)), "links": links, "points": int(coord.shape[0]),
       "steps": a.steps, "warmup": a.warmup,
       "phases": {k: spread([m[k] for m in phases]) for k in phases[0]},
       "call_wall": spread(calls),   # the Python call: the phases plus the copy of the link rows
       "host_link_share_of_total": float(np.mean([m["links"] / m["total"] for m in phases])),
       "yardstick": {"d8hdisttostrm": spread(dist_ms), "gagewatershed": spread(gage_ms)},
       "length_sweep_over_d8hdisttostrm": float(np.mean([m["length"] for m in phases]) / np.mean(dist_ms)),
       "label_sweep_over_gagewatershed": float(np.mean([m["label"] for m in phases]) / np.mean(gage_ms))}
write(res)
