"""SinmapSI on one MI355X, HBM-resident: slp and sca are the project's own dinfflowdir / areadinf of the synthetic DEM (Context.synth_dem, pit-filled), the
slope scaled so that the median of its positive values is the goldens' (0.7: the committed cases' slopes times 2.5 - the synthetic DEM at this size is
gentler than they are, and unscaled every cell is stable), four regions in vertical bands with the goldens' parameters (tests/sinmap_model.py: CALPAR, RMINTER, RMAXTER, RHOW),
road rasters that are non-zero on a fifth of the cells.  Timed, alternating call by call after a warm-up of each, the median of the library-side HIP-event
times of `--reps` calls: the library's two passes (classify, then the integrals on
the compacted list of cells) and the one-pass variant (TDX_SINMAP_ONEPASS), each without and with roads; and a device-to-device copy that moves the same total bytes (without roads 10 B read
+ 8 B written per cell: a copy of 9 B per cell; with roads 18 + 8: a copy of 13 B per cell), timed with events around it.  One JSON line: each time, the
ratio to the copy, Gcells/s, the share of cells per path, whether the variants gave the same bits.  No file of the reference is read; --ref-4096-s
records the reference tool's own printed "Compute time" at 4096 x 4096 (tests/golden/make_golden_sinmap.py --time-4096) next to the numbers.
--slope-scale S multiplies the slope by S instead (2.5 at 16384: every cell stable or flat, no cell reaches the integrals).
usage: python scripts/bench_sinmap.py [--size 16384] [--reps 11] [--slope-scale S] [--ref-4096-s S] [--out profiles/NAME.json]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import taudem_amd as T

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=16384)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--slope-scale", type=float, default=None)
ap.add_argument("--ref-4096-s", type=float, default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n = a.size
REGIONS = [(1, 2.0, 3.0, 0.0, 0.25, 30.0, 45.0, 2000.0), (2, 0.8, 4.5, 0.05, 0.4, 25.0, 38.0, 1800.0), (7, 1.5, 1.5, 0.1, 0.1, 28.0, 40.0, 2200.0),
           (300, 2.5, 2.9, 0.0, 0.15, 35.0, 35.0, 1600.0)]
RMINTER, RMAXTER, G, RHOW, SLOPE_MEDIAN = 0.0009, 0.00135, 9.81, 1000.0, 0.7
ctx = T.Context(0)
dem = ctx.synth_dem(n, seed=1234)
fel = ctx.pitremove(dem, -9999.0)
del dem
ang, slp = ctx.dinfflowdir(fel, -3.0e38, 30.0, 30.0)
del fel
sca = ctx.areadinf(ang, dx=30.0, dy=30.0)
del ang
SLOPE_SCALE = a.slope_scale if a.slope_scale else SLOPE_MEDIAN / float(slp[::16, ::16][slp[::16, ::16] > 0].median().item())   # (every 16th row and column: the median of a 1/256 sample)
slp = torch.where(slp == -1.0, slp, slp * SLOPE_SCALE).contiguous()
cal = torch.empty((n, n), dtype=torch.int16, device=slp.device)
for b, r in enumerate(REGIONS):
    cal[:, b * n // 4:(b + 1) * n // 4] = r[0]
gen = torch.Generator(device=slp.device).manual_seed(77)
on = torch.rand((n, n), generator=gen, device=slp.device) < 0.2
scamin = torch.where(on, torch.rand((n, n), generator=gen, device=slp.device) * 0.02, torch.zeros((), device=slp.device)).contiguous()
scamax = torch.where(on, scamin + torch.rand((n, n), generator=gen, device=slp.device) * 0.05, torch.zeros((), device=slp.device)).contiguous()
del on
si, sat = torch.empty_like(slp), torch.empty_like(slp)
ENVS = {"compact": None, "onepass": "TDX_SINMAP_ONEPASS"}


def run(variant, roads):
    for e in ENVS.values():
        if e:
            os.environ.pop(e, None)
    if ENVS[variant]:
        os.environ[ENVS[variant]] = "1"
    out = ctx.sinmapsi(slp, sca, cal, REGIONS, RMINTER, RMAXTER, G, RHOW, scamin=scamin if roads else None, scamax=scamax if roads else None, out=(si, sat), stats=True)
    return out[-1]["ms_total"]


def digest():
    torch.cuda.synchronize()
    return (int(si.view(torch.int32).to(torch.int64).sum().item()), int(sat.view(torch.int32).to(torch.int64).sum().item()))


def copy_ms(bytes_per_cell):
    src = torch.empty(n * n * bytes_per_cell, dtype=torch.uint8, device=slp.device).fill_(3)
    dst = torch.empty_like(src)
    dst.copy_(src)
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


names = [(v, roads) for roads in (False, True) for v in ENVS]
digests = {}
for v, roads in names:   # warm-up: code objects, scratch; and the bits of each variant
    run(v, roads)
    digests[(v, roads)] = digest()
run("onepass", False)
torch.cuda.synchronize()
live = ~((si == -1.0) & (sat == -1.0))
flat = live & (slp == 0.0)
rest = live & ~flat
shares = {"nodata": float((~live).float().mean().item()), "s_eq_0": float(flat.float().mean().item()), "unstable": float((rest & (si == 0.0)).float().mean().item()),
          "stable": float((rest & (si >= 1.0)).float().mean().item())}
reg = rest & (si != 0.0) & ~(si >= 1.0)
shares.update({"region1": float((reg & (sat == 3.0)).float().mean().item()), "region2": float((reg & (sat == 2.0)).float().mean().item()),
               "region3": float((reg & (sat < 2.0)).float().mean().item())})
del live, flat, rest, reg
times = {k: [] for k in names}
for _ in range(a.reps):
    for k in names:
        times[k].append(run(*k))
key = lambda v, roads: v + ("_roads" if roads else "")  # noqa: E731
ms = {key(*k): statistics.median(t) for k, t in times.items()}
copies = {"copy_9B": copy_ms(9), "copy_13B": copy_ms(13)}
cells = float(n) * float(n)
res = {"size": n, "reps": a.reps, "slope_scale": SLOPE_SCALE, "device": torch.cuda.get_device_name(0), "ms": ms, "ms_min": {key(*k): min(t) for k, t in times.items()},
       "ms_max": {key(*k): max(t) for k, t in times.items()}, "copy_ms": copies,
       "ratio_to_copy": {k: v / copies["copy_13B" if k.endswith("_roads") else "copy_9B"] for k, v in ms.items()},
       "gcells_per_s": {k: cells / v / 1e6 for k, v in ms.items()}, "path_shares_noroads": shares,
       "heavy_share_noroads": shares["region1"] + shares["region2"] + shares["region3"],
       "same_bits": {"noroads": len({digests[(v, False)] for v in ENVS}) == 1, "roads": len({digests[(v, True)] for v in ENVS}) == 1},
       "compact_over_onepass": ms["compact"] / ms["onepass"],
       "reference_compute_s_4096_one_rank": a.ref_4096_s}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
