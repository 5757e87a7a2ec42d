"""AreaD8's tile-contraction path with the clean tiles counted by pointer doubling (ad8_tile_fast_kernel) and the others redone by the Kahn sweep
(ad8_tile_local_kernel over the redo list): bit for bit against the restatement with contamination checking on and off, by default and with
TDX_AD8_LOCAL=kahn (every tile to the Kahn sweep), and the number of redone tiles (tdx_context_ad8_tile_counters) against a numpy predicate of "clean"
evaluated on the same p per 64 x 64 tile - all 64 rows in the raster, the tile and the ring around it inside the raster, every code there 1 .. 8, no
planted cycle - so that the fast kernel is neither silently unused nor used where it must not be.  A partial last tile row is not clean, whatever
lies below it."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits_equal, describe_diff

pytestmark = pytest.mark.gpu
TS = 64


def _p_field(oracle, shape, seed):
    dem = oracle.synth_dem(shape, seed)
    fel = oracle.pitremove(dem, -9999.0)
    p, _, _ = oracle.d8flowdir(fel, -3.0e38, 30.0, 30.0)
    return p


def _tiles(p):
    return -(-p.shape[0] // TS), -(-p.shape[1] // TS)


def _clean_tiles(p, cyclic=()):
    """The set of (ty, tx) that the fast kernel must finish."""
    ny, nx = p.shape
    tiles_y, tiles_x = _tiles(p)
    clean = set()
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            y0, x0 = ty * TS, tx * TS
            if y0 < 1 or x0 < 1 or y0 + TS > ny - 1 or x0 + TS > nx - 1 or (ty, tx) in cyclic:
                continue
            w = p[y0 - 1:y0 + TS + 1, x0 - 1:x0 + TS + 1]
            if ((w >= 1) & (w <= 8)).all():
                clean.add((ty, tx))
    return clean


def _counters(ctx):
    from taudem_amd import _lib

    fast, redone = C.c_int64(), C.c_int64()
    _lib.load().tdx_context_ad8_tile_counters(ctx._h, C.byref(fast), C.byref(redone))
    return fast.value, redone.value


def _check(ctx, oracle, monkeypatch, p, clean, name):
    tiles_y, tiles_x = _tiles(p)
    ntiles = tiles_y * tiles_x
    for cc in (True, False):
        a_o = oracle.aread8(p, -32768, contcheck=cc)
        monkeypatch.delenv("TDX_AD8_LOCAL", raising=False)
        a = ctx.aread8(p, -32768, contcheck=cc)
        fast, redone = _counters(ctx)
        monkeypatch.setenv("TDX_AD8_LOCAL", "kahn")
        a_k = ctx.aread8(p, -32768, contcheck=cc)
        fast_k, redone_k = _counters(ctx)
        monkeypatch.delenv("TDX_AD8_LOCAL", raising=False)
        assert bits_equal(a_k, a_o), describe_diff(a_k, a_o, f"{name}: Kahn sweep on every tile, contcheck={cc}")
        assert bits_equal(a, a_o), describe_diff(a, a_o, f"{name}: default, contcheck={cc}")
        assert (fast, redone) == (len(clean), ntiles - len(clean)), f"{name}: fast / redone tiles"
        assert (fast_k, redone_k) == (0, ntiles)


@pytest.mark.parametrize("shape,seed,interior", [((200, 333), 3, 8), ((777, 1000), 4, 154)])
def test_restatement_directions(shape, seed, interior, ctx, oracle, monkeypatch):
    p = _p_field(oracle, shape, seed)
    ty, tx = _tiles(p)
    # tiles with all 64 rows whose window lies inside the raster: 2 x 4 of the 4 x 6 tiles of (200, 333), whose last tile row has 8 rows, and 11 x 14 of the
    # 13 x 16 tiles of (777, 1000), whose last tile row has 9
    assert sum(1 for y in range(1, ty) for x in range(1, tx) if y * TS + TS <= shape[0] - 1 and x * TS + TS <= shape[1] - 1) == interior
    clean = _clean_tiles(p)
    assert len(clean) >= interior // 2, "the restatement's directions leave most interior tiles clean"
    _check(ctx, oracle, monkeypatch, p, clean, f"{shape}")


def _snake():
    """192 x 192, everything flows east, but the centre tile is one boustrophedon path through all its 4096 cells: 4095 hops, then out to the south."""
    p = np.full((192, 192), 1, dtype=np.int16)
    for ly in range(TS):
        even = ly % 2 == 0
        p[TS + ly, TS:2 * TS] = 1 if even else 5
        p[TS + ly, 2 * TS - 1 if even else TS] = 7
    return p


def test_longest_possible_path(ctx, oracle, monkeypatch):
    """The path needs exactly 12 doubling rounds - the cap: one more hop would be a cycle - and the tile must be counted as fast."""
    p = _snake()
    clean = _clean_tiles(p)
    assert clean == {(1, 1)}
    _check(ctx, oracle, monkeypatch, p, clean, "snake")
    a = ctx.aread8(p, -32768, contcheck=False)
    assert a[2 * TS - 1, TS] == 2 * 4096.0, "the path's last cell: the 4096 cells of the tile and, entering row by row from the west, the 64 x 64 cells of the tile beside it"


def test_quirks_in_interior_tiles(ctx, oracle, monkeypatch):
    """Each quirk in an interior tile of its own: a p == 0 cell, a nodata cell, a code 13, a p == 0 cell on a tile's rim (the ring of the tile above sees it too),
    and a 2-cycle in an otherwise clean tile, which the round cap sends to the redo list."""
    p = _p_field(oracle, (320, 320), 12).copy()
    before = _clean_tiles(p)
    assert before == {(y, x) for y in (1, 2, 3) for x in (1, 2, 3)}, "the restatement's directions leave every interior tile clean"
    p[1 * TS + 30, 1 * TS + 30] = 0
    p[1 * TS + 30, 3 * TS + 30] = -32768
    p[3 * TS + 30, 1 * TS + 30] = 13
    p[2 * TS, 2 * TS + 20] = 0                      # first row of tile (2, 2): in the ring of tile (1, 2)
    y, x = 3 * TS + 30, 3 * TS + 30
    p[y, x] = 1; p[y, x + 1] = 5                    # 2-cycle in tile (3, 3)
    clean = _clean_tiles(p, cyclic={(3, 3)})
    assert clean == {(2, 1), (2, 3), (3, 2)}
    _check(ctx, oracle, monkeypatch, p, clean, "quirks")


def test_three_strips(ctx, oracle, monkeypatch):
    """Strip heights 133, 133, 134: no multiple of 64, the ring rows of a strip's first and last tile rows come from the halo.  No redo count is asserted here."""
    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows
    import torch

    ny, nx, size = 400, 260, 3
    p = _p_field(oracle, (ny, nx), 21)
    ref = {cc: oracle.aread8(p, -32768, contcheck=cc) for cc in (True, False)}
    parts = partition_rows(ny, size)
    assert all((y1 - y0) % TS for y0, y1 in parts)
    p_t = torch.from_numpy(p)
    for mode in ("default", "kahn"):
        if mode == "kahn":
            monkeypatch.setenv("TDX_AD8_LOCAL", "kahn")
        else:
            monkeypatch.delenv("TDX_AD8_LOCAL", raising=False)
        with StripGroup(size, nx) as grp:
            def rank_main(r, c, comm):
                y0, y1 = parts[r]
                pipe = StripPipeline(c, comm, nx, y1 - y0)
                pp = pipe.empty(torch.int16)
                pp[1:y1 - y0 + 1].copy_(p_t[y0:y1])
                out = {}
                for cc in (True, False):
                    a, _ = pipe.aread8(pp, -32768, contcheck=cc)
                    torch.cuda.synchronize()
                    out[cc] = a[1:y1 - y0 + 1].cpu().numpy()
                return out
            res = grp.run(rank_main)
        for cc in (True, False):
            got = np.concatenate([r[cc] for r in res])
            assert bits_equal(got, ref[cc]), describe_diff(got, ref[cc], f"three strips, {mode}, contcheck={cc}")
    monkeypatch.delenv("TDX_AD8_LOCAL", raising=False)
