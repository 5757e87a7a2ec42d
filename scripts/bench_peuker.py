"""PeukerDouglas on one MI355X, HBM-resident: a synthetic DEM (Context.synth_dem), the fused kernel against the two-kernel path (TDX_PEUKER_TWOPASS, read
per call) in the same process, the two alternating call by call after a warm-up of each; the median of the library-side HIP-event times of `--reps` calls.
One JSON line: ms and Gcells/s of the fused kernel (ss alone and with the float copy w) and of the two-kernel path, their ratio, the fused kernel's
algorithmic bytes (4 read + 2 written per cell, + 4 with w; the two-kernel path moves about 14) over its time in GB/s and as a share of the 8 TB/s HBM
peak the project's roofline figures use (the D8 slope stencil, the project's streaming yardstick, reaches 53-55 % of it), and whether the two paths gave
the same bits.  No file of the reference is read.
usage: python scripts/bench_peuker.py [--size 16384] [--reps 21] [--out profiles/NAME.json]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import taudem_amd as T

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=16384)
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n = a.size
HBM_PEAK_GBS = 8000.0
ctx = T.Context(0)
fel = ctx.synth_dem(n, seed=7)
ss, w = torch.empty((n, n), dtype=torch.int16, device=fel.device), torch.empty((n, n), dtype=torch.float32, device=fel.device)


def run(twopass, float_weights):
    if twopass:
        os.environ["TDX_PEUKER_TWOPASS"] = "1"
    else:
        os.environ.pop("TDX_PEUKER_TWOPASS", None)
    out = ctx.peukerdouglas(fel, float_weights=float_weights, out=(ss, w) if float_weights else ss, stats=True)
    return out[-1]["ms_total"]


variants = {"fused": (False, False), "fused_w": (False, True), "twopass": (True, False), "twopass_w": (True, True)}
same = {}
for name, v in variants.items():   # warm-up: code objects, scratch; and the bits of each variant
    run(*v)
    torch.cuda.synchronize()
    same[name] = (int(ss.sum().item()), int((ss.to(torch.int64) * torch.arange(n, device=ss.device)[None, :]).sum().item()))
times = {name: [] for name in variants}
for _ in range(a.reps):
    for name, v in variants.items():
        times[name].append(run(*v))
ms = {name: statistics.median(t) for name, t in times.items()}
cells = float(n) * float(n)
res = {"size": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "flagged": same["fused"][0], "same_bits": len(set(same.values())) == 1,
       "ms": ms, "ms_min": {k: min(t) for k, t in times.items()}, "ms_max": {k: max(t) for k, t in times.items()},
       "gcells_per_s": {k: cells / v / 1e6 for k, v in ms.items()},
       "fused_gb_per_s": 6.0 * cells / ms["fused"] / 1e6, "fused_share_of_hbm_peak": 6.0 * cells / ms["fused"] / 1e6 / HBM_PEAK_GBS,
       "fused_w_gb_per_s": 10.0 * cells / ms["fused_w"] / 1e6, "fused_w_share_of_hbm_peak": 10.0 * cells / ms["fused_w"] / 1e6 / HBM_PEAK_GBS,
       "twopass_over_fused": ms["twopass"] / ms["fused"]}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
