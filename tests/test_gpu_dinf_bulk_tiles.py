"""The small-tile geometries of the D-infinity dependency sweep (16 x 16 one-wave tiles: AreaDinf's default from 2^29 cells per strip on; 32 x 32 tiles) on a
raster small enough for the suite.  TDX_DINF_BULK_TILE and TDX_DINF_BULK_UNTIL are read once per process, so each geometry runs in a child process that starts
with them set (the pattern of test_gpu_dropan.py::test_small_tiles_in_a_process_of_their_own); this process, where 25 tiles of 32 x 32 are fewer than the 400 at
which a bulk phase ends, runs on 64 x 64 tiles only and is held to the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, bits_equal, describe_diff

pytestmark = pytest.mark.gpu
ANG_ND = -3.402823466e38
NY, NX = 150, 130   # 10 x 9 tiles of 16, 5 x 5 of 32, 3 x 3 of 64: partial edge tiles in every geometry
KEYS = ("sca", "sca_w", "dsca")

# what a child runs: the three calls on one strip, then on two strips (45 tiles of 16 each: a bulk phase there too, followed by the exchange at once)
CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, {root!r})
import taudem_amd as T
from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows
a = np.load({inp!r})
ang, w, dm, outl = a['ang'], a['w'], a['dm'], (a['ox'], a['oy'])
ND = {nd!r}
out = {{}}
with T.Context(0) as c:
    out['sca_1'] = c.areadinf(ang, ND, 30.0, 30.0)
    out['sca_w_1'] = c.areadinf(ang, ND, 30.0, 30.0, weights=w, contcheck=False)
    out['dsca_1'] = c.dinfdecayaccum(ang, dm, ND, -9999.0, 30.0, 30.0, weights=w, contcheck=False, outlets=outl)
ny, nx = ang.shape
parts = partition_rows(ny, 2)
with StripGroup(2, nx, [0, 0]) as grp:
    def rank_main(r, c, comm):
        y0, y1 = parts[r]
        pipe = StripPipeline(c, comm, nx, y1 - y0)
        sl = slice(1, y1 - y0 + 1)
        def put(x):
            t = pipe.empty(torch.float32)
            t[sl] = torch.from_numpy(np.ascontiguousarray(x[y0:y1])).cuda()
            return t
        at, wt, dmt = put(ang), put(w), put(dm)
        s, _ = pipe.areadinf(at, ND, 30.0, 30.0)
        sw, _ = pipe.areadinf(at, ND, 30.0, 30.0, weights=wt, contcheck=False)
        d, _ = pipe.dinfdecayaccum(at, dmt, dx=30.0, dy=30.0, weights=wt, contcheck=False, outlets=pipe.local_outlets(outl[0], outl[1], y0))
        return [v[sl].cpu().numpy() for v in (s, sw, d)]
    res = grp.run(rank_main)
for i, k in enumerate(('sca', 'sca_w', 'dsca')):
    out[k + '_2'] = np.concatenate([r[i] for r in res], axis=0)
np.savez({outp!r}, **out)
"""


@pytest.fixture(scope="module")
def case(oracle):
    rng = np.random.default_rng(1607)
    dem = oracle.synth_dem((NY, NX), 77)
    dem[58:71, 40:62] = -9999.0   # one nodata hole, across the corner of four 16-tiles and the edge of two 32-tiles
    fel = oracle.pitremove(dem, -9999.0)
    ang, _, _ = oracle.dinfflowdir(fel, -3.0e38, 30.0, 30.0)
    w = rng.random((NY, NX), dtype=np.float32) + np.float32(0.25)
    dm = (rng.random((NY, NX), dtype=np.float32) * np.float32(0.1) + np.float32(0.9)).astype(np.float32)
    sca_nc = oracle.areadinf(ang, ANG_ND, 30.0, 30.0, contcheck=False)
    pick = rng.choice(np.argsort(sca_nc, axis=None)[-60:], size=3, replace=False)   # three outlets on cells of large area
    oy, ox = np.unravel_index(pick, sca_nc.shape)
    outl = (ox.astype(np.int32), oy.astype(np.int32))
    ref = {"sca": oracle.areadinf(ang, ANG_ND, 30.0, 30.0),
           "sca_w": oracle.areadinf(ang, ANG_ND, 30.0, 30.0, weights=w, contcheck=False),
           "dsca": oracle.dinfdecayaccum(ang, dm, ANG_ND, -9999.0, 30.0, 30.0, weights=w, contcheck=False, outlets=outl)}
    return {"ang": ang, "w": w, "dm": dm, "outl": outl, "ref": ref}


def _three_calls(ctx, case):
    ang, w, dm, outl = case["ang"], case["w"], case["dm"], case["outl"]
    return {"sca": ctx.areadinf(ang, ANG_ND, 30.0, 30.0),
            "sca_w": ctx.areadinf(ang, ANG_ND, 30.0, 30.0, weights=w, contcheck=False),
            "dsca": ctx.dinfdecayaccum(ang, dm, ANG_ND, -9999.0, 30.0, 30.0, weights=w, contcheck=False, outlets=outl)}


@pytest.fixture(scope="module")
def mine(ctx, case):
    """This process' rasters (64 x 64 tiles only), equal to the oracle's bit for bit; the children are compared with these."""
    got = _three_calls(ctx, case)
    for k in KEYS:
        assert bits_equal(got[k], case["ref"][k]), describe_diff(got[k], case["ref"][k], f"64 x 64 tiles: {k}")
    return got


def test_walk_equals_sweep(ctx, case, mine, monkeypatch):
    monkeypatch.setenv("TDX_DINF_WALK", "1")   # read per call
    got = _three_calls(ctx, case)
    for k in KEYS:
        assert bits_equal(got[k], mine[k]), describe_diff(got[k], mine[k], f"atomic walk: {k}")


@pytest.mark.parametrize("edge,ntiles", [(16, 90), (32, 25)])
def test_bulk_tiles_in_a_process_of_their_own(edge, ntiles, case, mine, tmp_path):
    """Bulk rounds on `edge` x `edge` tiles until a round has at most 20 active tiles, the hand-over to the 3 x 3 tiles of 64, on one strip and on two (two rounds
    between exchanges), all under the sweep verifier: every raster equals this process', bit for bit."""
    np.savez(tmp_path / "in.npz", ang=case["ang"], w=case["w"], dm=case["dm"], ox=case["outl"][0], oy=case["outl"][1])
    code = CHILD.format(root=ROOT, inp=str(tmp_path / "in.npz"), outp=str(tmp_path / "out.npz"), nd=ANG_ND)
    env = dict(os.environ, TDX_DINF_BULK_TILE=str(edge), TDX_DINF_BULK_UNTIL="20", TDX_SWEEP_VERIFY="1", TDX_DEBUG_ROUNDS="2", TDX_SWEEP_EAGER_ROUNDS="2")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.load(tmp_path / "out.npz")
    for k in KEYS:
        for strips in ("1", "2"):
            assert bits_equal(out[f"{k}_{strips}"], mine[k]), describe_diff(out[f"{k}_{strips}"], mine[k], f"{edge} x {edge} bulk tiles, {strips} strip(s): {k}")
    lines = r.stderr.splitlines()
    small = f"dinf sweep rounds({ntiles} tiles of {edge}):"
    assert any(ln.startswith(small) for ln in lines), f"no bulk phase on {ntiles} tiles of {edge}:\n{r.stderr}"
    assert any(ln.startswith("dinf sweep rounds(9 tiles of 64):") for ln in lines), f"no hand-over to the 64 x 64 tiles:\n{r.stderr}"
    if edge == 16:   # a strip of 75 + 2 rows: 9 x 5 tiles of 16, more than 20 - the bulk phase that is followed by the exchange at once
        assert any(ln.startswith("dinf sweep rounds(45 tiles of 16):") for ln in lines), f"no bulk phase on the strips:\n{r.stderr}"
