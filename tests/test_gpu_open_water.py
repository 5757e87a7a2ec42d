"""The open-water blocks (flats.hpp: OPEN WATER; tile_relax.hpp: macro_role) on lakes whose block layout is known (tests/lakes.py, checked on the CPU by
tests/test_lakes.py): D8FlowDir and DinfFlowDir against the restatement bit for bit (ang: one float32 ulp, test_gpu_dinf.check_angles), and every case
shows that the blocks were used - fewer rounds than with TDX_FLATS_MACRO=0.

- the ring-position sweep: K = 2, 4, 8 x ring edge 0 .. 3 x positions 0, 1, 2, 63, 64, 65, 127, 128, 129, W - 1, W, W + 1 x incfall / incrise source
  (the closed form's beside / across / right-angle cases, the guards of its far terms, the corners, the waves' boundaries), with the largest block
  limited to 2, 4 and 8 tiles;
- raster shapes: both paths of find_blocks_kernel, blocks at the outermost tile rows and columns a block can take, partial tiles, undrained lakes,
  islands, a nodata shore, two blocks chained through each other's ring;
- lakes shaped for the moved[] flag race of LevelOpT::macro_update, twice in a row;
- one and four block workgroups per CU, the strided path of macro_role (first rounds of more than 4096 entries), strips, the int16 -> int32 restart."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lakes as LK
from conftest import bits_equal, describe_diff
from test_gpu_dinf import check_angles

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE = {}


def _oracle(oracle, key, z):
    if key not in _ORACLE:
        p, sd8, st = oracle.d8flowdir(z, -3.0e38, 30.0, 30.0)
        ang, slp, _ = oracle.dinfflowdir(z, -3.0e38, 30.0, 30.0)
        _ORACLE[key] = dict(p=p, sd8=sd8, ang=ang, slp=slp, flats=st["flats_initial"])
    return _ORACLE[key]


def _check(r, o, what):
    assert bits_equal(r["p"], o["p"]), describe_diff(r["p"], o["p"], f"p, {what}")
    assert bits_equal(r["sd8"], o["sd8"]), describe_diff(r["sd8"], o["sd8"], f"sd8, {what}")
    assert bits_equal(r["slp"], o["slp"]), describe_diff(r["slp"], o["slp"], f"slp, {what}")
    check_angles(r["ang"], o["ang"], f"ang, {what}")


def _run(ctx, z, monkeypatch, kmax=None):
    if kmax is None:
        monkeypatch.delenv("TDX_FLATS_MACRO", raising=False)
    else:
        monkeypatch.setenv("TDX_FLATS_MACRO", str(kmax))
    p, sd8, st = ctx.d8flowdir(z, -3.0e38, 30.0, 30.0, stats=True)
    ang, slp, std = ctx.dinfflowdir(z, -3.0e38, 30.0, 30.0, stats=True)
    monkeypatch.delenv("TDX_FLATS_MACRO", raising=False)
    return dict(p=p, sd8=sd8, ang=ang, slp=slp, rounds=st["rounds"], rounds_dinf=std["rounds"], flats=st["flats_initial"])


def _blocks_and_values(ctx, oracle, monkeypatch, key, z, kmaxes=(None,)):
    o = _oracle(oracle, key, z)
    plain = _run(ctx, z, monkeypatch, 0)
    _check(plain, o, f"{key}, no blocks")
    assert plain["flats"] == o["flats"] > z.size // 16   # a dense first queue: DinfFlowDir uses the blocks too
    out = None
    for km in kmaxes:
        r = _run(ctx, z, monkeypatch, km)
        _check(r, o, f"{key}, blocks <= {km or 8}")
        assert r["rounds"] < plain["rounds"] and r["rounds_dinf"] < plain["rounds_dinf"], f"{key}, blocks <= {km or 8}: the blocks were not used"
        out = out or r
    return o, out


@pytest.mark.parametrize("source", ["fall", "rise"])
@pytest.mark.parametrize("k", [2, 4, pytest.param(8, marks=pytest.mark.slow)])
def test_ring_position_sweep(ctx, oracle, monkeypatch, k, source):
    z, lakes = LK.sweep_raster(k, source)
    assert len(lakes) == 4 * len(LK.positions(k))
    _blocks_and_values(ctx, oracle, monkeypatch, f"sweep{k}{source}", z, kmaxes=[None] + [km for km in (2, 4) if km <= k])


@pytest.mark.parametrize("name", sorted(LK.SHAPES))
def test_shapes(ctx, oracle, monkeypatch, name):
    z, lakes = LK.shapes_raster(name)
    _blocks_and_values(ctx, oracle, monkeypatch, f"shape{name}", z)


def _race_raster():
    return LK.race_raster()[0]


def test_race_shaped_lakes_twice(ctx, oracle, monkeypatch):
    """lakes where a lost moved[4 + E] flag (LevelOpT::macro_update) would leave wrong levels for good; the same bits in two runs"""
    z = _race_raster()
    o, first = _blocks_and_values(ctx, oracle, monkeypatch, "race", z)
    again = _run(ctx, z, monkeypatch)
    for key in ("p", "sd8", "ang", "slp"):
        assert bits_equal(again[key], first[key]), describe_diff(again[key], first[key], f"{key}, second run")


def _subprocess_run(tmp_path, z, env):
    np.save(tmp_path / "z.npy", z)
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "open_water_worker.py"), str(tmp_path / "z.npy"), str(tmp_path / "out.npz")], env=e,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    g = np.load(tmp_path / "out.npz")
    return {k: g[k] for k in g.files}


@pytest.mark.parametrize("wgs", ["1", "4"])
def test_block_workgroups(ctx, oracle, tmp_path, wgs):
    """TDX_MACRO_WGS (block workgroups per CU, read once per process): one and the default four"""
    z = _race_raster()
    r = _subprocess_run(tmp_path, z, {"TDX_MACRO_WGS": wgs})
    _check(r, _oracle(oracle, "race", z), f"TDX_MACRO_WGS={wgs}")


def test_int16_to_int32_restart(ctx, oracle, tmp_path):
    """TDX_LEVELS_LIMIT below the lakes' deepest level: the int16 pass (blocks on) gives up and the call starts over on int32 fields"""
    z, lakes = LK.sweep_raster(4, "fall")
    r = _subprocess_run(tmp_path, z, {"TDX_LEVELS_LIMIT": "100"})
    assert int(r["levels"]) > 100
    _check(r, _oracle(oracle, "sweep4fall", z), "TDX_LEVELS_LIMIT=100")


@pytest.mark.slow
def test_strided_macro_role(ctx, oracle, monkeypatch):
    """a raster whose first rounds hold more than 4096 list entries AND blocks: macro_role's strided path (rough ground: a pit in nearly every tile)"""
    lakes = [LK.Lake(k, rx * 8 + {2: 2, 4: 4, 8: 0}[k], ry * 8 + {2: 2, 4: 4, 8: 0}[k], fall=((E, j),))
             for n, (k, rx, ry, E, j) in enumerate([(2, 0, 0, 0, 64), (4, 2, 0, 1, 128), (8, 5, 1, 2, 1), (2, 8, 0, 3, 129), (4, 0, 4, 0, 0),
                                                    (8, 3, 3, 1, 300), (2, 7, 5, 2, 65), (4, 2, 7, 3, 257), (8, 7, 7, 0, 511), (2, 4, 8, 1, 2)])]
    z = LK.make_dem((5120, 5120), lakes, rough=0.5, seed=7)
    c = LK.classify(z)
    blocks, owner = LK.find_blocks(LK.full_tiles(c["fm"]))
    assert len(blocks) >= len(lakes) and LK.first_round_entries(c["q"], blocks, owner) > 4096
    _blocks_and_values(ctx, oracle, monkeypatch, "strided", z)


@pytest.mark.parametrize("cuts", [(64 * 20 + 1,), (64 * 7 + 63, 64 * 33), (64 * 4 + 65, 512 * 2 + 256, 64 * 25 + 1, 64 * 40 + 63)],
                         ids=["2strips", "3strips", "5strips"])
def test_strips(ctx, oracle, monkeypatch, cuts):
    """2, 3 and 5 strips cut at rows = 1, 63, 0, 65 (mod 64) and through the middle of an 8 x 8-tile region (a block's rows next to a strip boundary stay
    ordinary tiles): the same bits as one strip and as the restatement"""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline

    z, lakes = LK.sweep_raster(4, "fall")
    ny, nx = z.shape
    o, one = _blocks_and_values(ctx, oracle, monkeypatch, "sweep4fall", z)
    edges = [0, *cuts, ny]
    parts = list(zip(edges[:-1], edges[1:]))
    zt = torch.from_numpy(z)
    with StripGroup(len(parts), nx) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            pipe = StripPipeline(c, comm, nx, y1 - y0)
            f = pipe.empty(torch.float32)
            f[1:y1 - y0 + 1].copy_(zt[y0:y1])
            pp, ss, _ = pipe.d8flowdir(f, -3.0e38, 30.0, 30.0)
            aa, sl, _ = pipe.dinfflowdir(f, -3.0e38, 30.0, 30.0)
            torch.cuda.synchronize()
            return [t[1:y1 - y0 + 1].cpu().numpy() for t in (pp, ss, aa, sl)]
        res = grp.run(rank_main)
    r = {key: np.concatenate([x[i] for x in res]) for i, key in enumerate(("p", "sd8", "ang", "slp"))}
    _check(r, o, f"{len(parts)} strips")
    for key in ("p", "sd8", "ang", "slp"):
        assert bits_equal(r[key], one[key]), describe_diff(r[key], one[key], f"{key}: {len(parts)} strips against one")
