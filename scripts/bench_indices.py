"""The terrain-index kernels on one MI355X, HBM-resident.  slp and sca are the project's own dinfflowdir / areadinf of the synthetic DEM (Context.synth_dem,
pit-filled), plen and ad8 its d8flowdir -> gridnet / aread8, p that d8flowdir's with a tenth of the raster cut out in 64 x 64 blocks of nodata, gw a grid that
has data outside those blocks on nine cells in ten - so the cells inside the blocks, and a tenth of the others, are SetRegion's holes.  Timed, alternating
call by call after a warm-up of each, with the library-side HIP-event time of `--reps` calls each (median, min, max):

    twi, sa, sar      terrain_indices with one output (8 B read + 4 B written per cell)
    fused3            terrain_indices with all three (8 + 12 B)
    seq3              the three one-output calls one after the other, their times added (24 + 12 B)
    lengtharea        8 B read + 2 B written
    setregion         6 B read + 4 B written, and the neighbour reads of the holes

and for each a device-to-device copy that moves the same total bytes (a copy of half that many), timed with events around it.  One JSON line: the times,
the ratio of each to its copy, Gcells/s, the share of hole cells, whether fused3 gave the bits of the one-output calls.  No file of the reference is read.
usage: python scripts/bench_indices.py [--size 16384] [--reps 11] [--out profiles/NAME.json]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import taudem_amd as T

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=16384)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n = a.size
M_EXP, N_EXP, LA_M, LA_Y = 2.0, 1.0, 0.03, 1.3   # the reference's -par defaults
ctx = T.Context(0)
dem = ctx.synth_dem(n, seed=1234)
fel = ctx.pitremove(dem, -9999.0)
del dem
ang, slp = ctx.dinfflowdir(fel, -3.0e38, 30.0, 30.0)
sca = ctx.areadinf(ang, dx=30.0, dy=30.0)
del ang
p, _ = ctx.d8flowdir(fel, -3.0e38, 30.0, 30.0)
del fel, _
ad8 = ctx.aread8(p)
plen = ctx.gridnet(p, dx=30.0, dy=30.0)[0].contiguous()
dev = slp.device
rows = torch.arange(n, device=dev).view(n, 1) // 64
cols = torch.arange(n, device=dev).view(1, n) // 64
block = ((rows * 7 + cols * 3) % 10 == 0)
p = torch.where(block, torch.full((), -32768, dtype=torch.int16, device=dev), p).contiguous()
gen = torch.Generator(device=dev).manual_seed(77)
gw = torch.where(block | (torch.rand((n, n), generator=gen, device=dev) < 0.1), torch.full((), -2147483647, dtype=torch.int32, device=dev),
                 torch.ones((), dtype=torch.int32, device=dev)).contiguous()
hole_share = float(((p == -32768) & (gw == -2147483647)).float().mean().item())
del block, rows, cols
o = {k: torch.empty_like(slp) for k in ("twi", "sa", "sar", "f_twi", "f_sa", "f_sar")}
ss = torch.empty((n, n), dtype=torch.int16, device=dev)
reg = torch.empty((n, n), dtype=torch.int32, device=dev)


def ms(res):
    return res[-1]["ms_total"]


RUNS = {
    "twi": lambda: ms(ctx.twi(slp, sca, out=o["twi"], stats=True)),
    "sa": lambda: ms(ctx.slopearea(slp, sca, M_EXP, N_EXP, out=o["sa"], stats=True)),
    "sar": lambda: ms(ctx.slopearearatio(slp, sca, out=o["sar"], stats=True)),
    "fused3": lambda: ms(ctx.terrain_indices(slp, sca, M_EXP, N_EXP, out=(o["f_twi"], o["f_sa"], o["f_sar"]), stats=True)),
    "lengtharea": lambda: ms(ctx.lengtharea(plen, ad8, LA_M, LA_Y, out=ss, stats=True)),
    "setregion": lambda: ms(ctx.setregion(p, gw, 1, out=reg, stats=True)),
}
RUNS["seq3"] = lambda: RUNS["twi"]() + RUNS["sa"]() + RUNS["sar"]()
COPY_BYTES = {"twi": 6, "sa": 6, "sar": 6, "fused3": 10, "seq3": 18, "lengtharea": 5, "setregion": 5}   # half the bytes the call reads and writes per cell


def copy_ms(bytes_per_cell):
    src = torch.empty(n * n * bytes_per_cell, dtype=torch.uint8, device=dev).fill_(3)
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


for f in RUNS.values():   # warm-up: code objects
    f()
torch.cuda.synchronize()
same = all(torch.equal(o[k].view(torch.int32), o["f_" + k].view(torch.int32)) for k in ("twi", "sa", "sar"))
times = {k: [] for k in RUNS}
for _ in range(a.reps):
    for k, f in RUNS.items():
        times[k].append(f())
med = {k: statistics.median(t) for k, t in times.items()}
copies = {f"copy_{b}B": copy_ms(b) for b in sorted(set(COPY_BYTES.values()))}
cells = float(n) * float(n)
res = {"size": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "par": {"m": M_EXP, "n": N_EXP, "M": LA_M, "y": LA_Y}, "ms": med,
       "ms_min": {k: min(t) for k, t in times.items()}, "ms_max": {k: max(t) for k, t in times.items()}, "copy_ms": copies,
       "ratio_to_copy": {k: v / copies[f"copy_{COPY_BYTES[k]}B"] for k, v in med.items()}, "gcells_per_s": {k: cells / v / 1e6 for k, v in med.items()},
       "fused3_over_seq3": med["fused3"] / med["seq3"], "setregion_hole_share": hole_share, "fused3_same_bits_as_single_calls": same,
       "twi_live_share": float((o["twi"] != -1.0).float().mean().item()), "ss_share_of_ones": float((ss == 1).float().mean().item())}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
