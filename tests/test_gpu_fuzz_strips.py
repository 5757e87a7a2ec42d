"""Seeded fuzz of the strip protocol (round 5: coarse levels across strips, tree-wise big-cell folds on pending lists, bounded sweep / closure rounds between
two exchanges, both level fields side by side): random raster shapes, rank counts (2 ... 8, strips shorter than a tile included), nodata holes, weights,
outlets and a lowered big-cell threshold - every raster of every tool must equal the pinned restatement's, bit for bit, whatever the cut."""
import os

import numpy as np
import pytest

from conftest import bits_equal, describe_diff

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
ANG_ND = -3.402823466e38


def _case(seed):
    rng = np.random.default_rng(1000 + seed)
    scale = int(os.environ.get("TDX_FUZZ_SCALE", "1"))
    ny = int(rng.integers(40, 700 * scale))
    nx = int(rng.integers(40, 900 * scale))
    world = int(rng.integers(2, 9))
    world = max(2, min(world, ny // 3))
    holes = int(rng.integers(0, 4))
    thr = int(rng.choice([3, 8, 40, 1 << 24]))
    eager = int(rng.choice([1, 2, 8]))
    return ny, nx, world, holes, thr, eager, rng


# (TDX_FUZZ_SEEDS=n: a longer one-off sweep, e.g. after a change of the strip protocol; TDX_FUZZ_SCALE=k: rasters up to k x larger on each side)
@pytest.mark.parametrize("seed", range(int(os.environ.get("TDX_FUZZ_SEEDS", "32"))))
def test_random_cut_random_raster(seed, oracle, monkeypatch):
    _fuzz(seed, oracle, monkeypatch, _case(seed), 30.0, 25.0, f"seed {seed}")


# Per-row cell sizes (tests/cellsizes.py): the coarse geographic band (70 N -> 40 N) and `wild` rows, each strip given its rows through
# taudem_amd.distributed.strip_rows - a halo row's sizes are those of the neighbouring global row - and the restatement the global rows.
# Seeds 100 + i: other shapes and cuts than the constant-size seeds above.
@pytest.mark.parametrize("kind", ["geographic", "wild"])
@pytest.mark.parametrize("seed", range(int(os.environ.get("TDX_FUZZ_SEEDS", "32")) // 2))
def test_random_cut_random_raster_per_row_sizes(seed, kind, oracle, monkeypatch):
    from cellsizes import rows

    case = _case(100 + seed)
    dx, dy = rows("band" if kind == "geographic" else "wild", case[0], seed=seed)
    _fuzz(100 + seed, oracle, monkeypatch, case, dx, dy, f"seed {100 + seed} ({kind} rows)")


def _fuzz(seed, oracle, monkeypatch, case, dx, dy, label):
    """dx, dy: scalars or the global per-row arrays."""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows, strip_rows

    ny, nx, world, holes, thr, eager, rng = case
    dem = oracle.synth_dem((ny, nx), 500 + seed)
    for _ in range(holes):
        y0, x0 = int(rng.integers(0, ny - 5)), int(rng.integers(0, nx - 5))
        dem[y0:y0 + int(rng.integers(2, ny // 3 + 3)), x0:x0 + int(rng.integers(2, nx // 3 + 3))] = -9999.0
    w = rng.random((ny, nx), dtype=np.float32) + np.float32(0.25)
    dm = (rng.random((ny, nx), dtype=np.float32) * np.float32(0.1) + np.float32(0.9)).astype(np.float32)
    fel_o = oracle.pitremove(dem, -9999.0)
    p_o, sd8_o, _ = oracle.d8flowdir(fel_o, -3.0e38, dx, dy)
    ang_o, slp_o, _ = oracle.dinfflowdir(fel_o, -3.0e38, dx, dy)
    a_o = oracle.aread8(p_o, -32768, contcheck=False)
    aw_o = oracle.aread8(p_o, -32768, weights=w, contcheck=True)
    sca_o = oracle.areadinf(ang_o, ANG_ND, dx, dy, contcheck=False)
    # outlets: a handful of cells with large D8 area (inside the raster, wherever they fall relative to the cut)
    flat = np.argsort(a_o, axis=None)[-400:]
    pick = rng.choice(flat, size=5, replace=False)
    oy, ox = np.unravel_index(pick, a_o.shape)
    outl = (ox.astype(np.int32), oy.astype(np.int32))
    ao_o = oracle.aread8(p_o, -32768, contcheck=False, outlets=outl)
    d_o = oracle.dinfdecayaccum(ang_o, dm, dx=dx, dy=dy, weights=w, contcheck=False, outlets=outl)
    # the reverse sweeps (round 6: a tile routine of their own): a disturbance grid of scattered cells, the weights as the accumulated quantity
    dg = (rng.random((ny, nx)) < 0.02).astype(np.int32)
    dep_o = oracle.dinfupdependence(ang_o, dg, dx=dx, dy=dy)
    racc_o, dmax_o = oracle.dinfrevaccum(ang_o, w, dx=dx, dy=dy)
    monkeypatch.setenv("TDX_AD8_BIG_THRESHOLD", str(thr))
    monkeypatch.setenv("TDX_SWEEP_EAGER_ROUNDS", str(eager))
    monkeypatch.setenv("TDX_REACH_EAGER_ROUNDS", str(eager))
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    parts = partition_rows(ny, world)
    with StripGroup(world, nx, [0] * world) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            nyl = y1 - y0
            pipe = StripPipeline(c, comm, nx, nyl)
            sl = slice(1, nyl + 1)
            sdx, sdy = strip_rows(dx, y0, y1), strip_rows(dy, y0, y1)

            def put(a, dt):
                t = pipe.empty(dt)
                t[sl] = torch.from_numpy(np.ascontiguousarray(a[y0:y1])).cuda()
                return t
            d = put(dem, torch.float32)
            fel, _ = pipe.pitremove(d, -9999.0)
            p, sd8, _ = pipe.d8flowdir(fel, -3.0e38, sdx, sdy)
            ang, slp, _ = pipe.dinfflowdir(fel, -3.0e38, sdx, sdy)
            wt, dmt = put(w, torch.float32), put(dm, torch.float32)
            a, _ = pipe.aread8(p, -32768, contcheck=False)
            aw, _ = pipe.aread8(p, -32768, weights=wt, contcheck=True)
            sca, _ = pipe.areadinf(ang, ANG_ND, sdx, sdy, contcheck=False)
            lo = pipe.local_outlets(outl[0], outl[1], y0)
            ao, _ = pipe.aread8(p, -32768, contcheck=False, outlets=lo)
            dd, _ = pipe.dinfdecayaccum(ang, dmt, dx=sdx, dy=sdy, weights=wt, contcheck=False, outlets=lo)
            dep, _ = pipe.dinfupdependence(ang, put(dg, torch.int32), dx=sdx, dy=sdy)
            racc, dmax, _ = pipe.dinfrevaccum(ang, wt, dx=sdx, dy=sdy)
            return {k: v[sl].cpu().numpy() for k, v in (("fel", fel), ("p", p), ("sd8", sd8), ("ang", ang), ("slp", slp), ("ad8", a), ("ad8_w", aw), ("sca", sca),
                                                        ("ad8_o", ao), ("dsca_o", dd), ("dep", dep), ("racc", racc), ("dmax", dmax))}
        res = grp.run(rank_main)
    what = f"{label}: {ny} x {nx} in {world} strips, {holes} holes, big-cell threshold {thr}, {eager} rounds between exchanges"
    for key, ref in (("fel", fel_o), ("p", p_o), ("sd8", sd8_o), ("ang", ang_o), ("slp", slp_o), ("ad8", a_o), ("ad8_w", aw_o), ("sca", sca_o), ("ad8_o", ao_o),
                     ("dsca_o", d_o), ("dep", dep_o), ("racc", racc_o), ("dmax", dmax_o)):
        got = np.concatenate([r[key] for r in res], axis=0)
        assert bits_equal(got, ref), describe_diff(got, ref, f"{what}: {key}")


# Every tool downstream of the directions under the random cut (tests/downstream.py: the strip entry points of DinfUpDependence,
# DinfRevAccum, DinfDecayAccum, DinfConcLimAccum, DinfTransLimAccum, DinfDistDown, DinfDistUp, D8HDistToStrm, GageWatershed, GridNet and
# D8FlowPathExtremeUp, plus the upstream strip tools), fed the oracle's directions of the global raster and held to the restatements of the
# global rasters and global per-row sizes; gauges and outlets on the cut rows, every rank's -id table equal to the restatement's -id text.
# Seeds 200 + i: other shapes and cuts than the seeds above; the distance modes rotate with i, every (stat, kind) within 12 seeds; cell
# sizes rotate through constant, `wild` and geographic `band` rows.
@pytest.fixture(scope="module")
def restate_downstream(tmp_path_factory, oracle):
    import downstream as D

    return D.Restate(tmp_path_factory.mktemp("downstream"), oracle)


@pytest.mark.parametrize("seed", range(int(os.environ.get("TDX_FUZZ_SEEDS", "32"))))
def test_random_cut_downstream_tools(seed, oracle, restate_downstream, monkeypatch):
    import torch

    import downstream as D
    from cellsizes import rows
    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows, strip_rows

    ny, nx, world, holes, thr, eager, rng = _case(200 + seed)
    dx, dy = [(30.0, 25.0), rows("wild", ny, seed=seed), rows("band", ny)][seed % 3]
    dem = oracle.synth_dem((ny, nx), 500 + 200 + seed)
    for _ in range(holes):
        y0, x0 = int(rng.integers(0, ny - 5)), int(rng.integers(0, nx - 5))
        dem[y0:y0 + int(rng.integers(2, ny // 3 + 3)), x0:x0 + int(rng.integers(2, nx // 3 + 3))] = -9999.0
    parts = partition_rows(ny, world)
    cut = sorted({y for y0, y1 in parts for y in (y0 - 1, y0, y1 - 1, y1) if 0 <= y < ny})
    inp = D.derive(oracle, dem, dx, dy, 3000 + seed, cut_rows=cut)
    ref = D.reference(restate_downstream, inp, dx, dy, seed)
    monkeypatch.setenv("TDX_AD8_BIG_THRESHOLD", str(thr))
    monkeypatch.setenv("TDX_SWEEP_EAGER_ROUNDS", str(eager))
    monkeypatch.setenv("TDX_REACH_EAGER_ROUNDS", str(eager))
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    with StripGroup(world, nx, [0] * world) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            nyl = y1 - y0
            pipe = StripPipeline(c, comm, nx, nyl)

            def put(a):
                t = pipe.empty(getattr(torch, np.asarray(a).dtype.name))
                t[1:nyl + 1] = torch.from_numpy(np.ascontiguousarray(a[y0:y1])).cuda()
                return t
            return D.strip(pipe, put, inp, strip_rows(dx, y0, y1), strip_rows(dy, y0, y1), y0, y1, seed)
        res = grp.run(rank_main)
    what = (f"seed {200 + seed}: {ny} x {nx} in {world} strips, {holes} holes, big-cell threshold {thr}, {eager} rounds between exchanges, "
            f"{['constant', 'wild', 'band'][seed % 3]} cell sizes")
    got = {k: np.concatenate([r[k] for r in res], axis=0) for k in res[0] if k != "gw_id"}
    bad = D.compare(got, {k: v for k, v in ref.items() if k != "gw_id"}, what)
    bad += [f"{what}: rank {r} -id table {res[r]['gw_id']!r} vs {ref['gw_id']!r}" for r in range(world) if res[r]["gw_id"] != ref["gw_id"]]
    assert not bad, "\n".join(bad)


# The five sweep tools that came after those - RetLimFlow, DinfAvalanche, FlowDirCond, D8VDistToStrm, SlopeAveDown - under the same draw of
# shape, rank count, holes and eager rounds (_case(300 + seed)): downstream.extras_late on derive()'s outlets-free inputs, the strip entry
# points against the restatements of the global rasters.  SlopeAveDown gets the whole raster's pass count and exchanges its record halos
# after every pass; DinfAvalanche gets each strip's first global row, the raster's height and, in -direct mode, the whole raster's geometry.
# The avalanche runs on 30 x 40 cells where the sizes are constant and on the `wild` / `band` rows themselves otherwise, with sources the
# restatement alone keeps inside the tainted share (tests/downstream.py).
@pytest.mark.parametrize("seed", range(int(os.environ.get("TDX_FUZZ_SEEDS", "32"))))
def test_random_cut_late_tools(seed, oracle, restate_downstream, monkeypatch):
    import torch

    import downstream as D
    from cellsizes import rows
    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows, strip_rows

    ny, nx, world, holes, thr, eager, rng = _case(300 + seed)
    dx, dy = [(30.0, 25.0), rows("wild", ny, seed=seed), rows("band", ny)][seed % 3]
    dem = oracle.synth_dem((ny, nx), 500 + 300 + seed)
    for _ in range(holes):
        y0, x0 = int(rng.integers(0, ny - 5)), int(rng.integers(0, nx - 5))
        dem[y0:y0 + int(rng.integers(2, ny // 3 + 3)), x0:x0 + int(rng.integers(2, nx // 3 + 3))] = -9999.0
    parts = partition_rows(ny, world)
    inp = D.extras_late(D.derive(oracle, dem, dx, dy, 4000 + seed), 4000 + seed, restate_downstream, dx, dy, seed)
    ref = D.reference_late(restate_downstream, inp, dx, dy, seed)
    dns = D.late_dns(dx, dy, seed)
    monkeypatch.setenv("TDX_SWEEP_EAGER_ROUNDS", str(eager))
    monkeypatch.setenv("TDX_REACH_EAGER_ROUNDS", str(eager))
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    with StripGroup(world, nx, [0] * world) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            nyl = y1 - y0
            pipe = StripPipeline(c, comm, nx, nyl)

            def put(a):
                t = pipe.empty(getattr(torch, np.asarray(a).dtype.name))
                t[1:nyl + 1] = torch.from_numpy(np.ascontiguousarray(a[y0:y1])).cuda()
                return t
            return D.strip_late(pipe, put, inp, strip_rows(dx, y0, y1), strip_rows(dy, y0, y1), y0, y1, ny, dns, seed)
        res = grp.run(rank_main)
    what = (f"seed {300 + seed}: {ny} x {nx} in {world} strips, {holes} holes, {eager} rounds between exchanges, "
            f"{['constant', 'wild', 'band'][seed % 3]} cell sizes")
    bad = D.compare_late({k: np.concatenate([r[k] for r in res], axis=0) for k in res[0]}, ref, what)
    assert not bad, "\n".join(bad)
