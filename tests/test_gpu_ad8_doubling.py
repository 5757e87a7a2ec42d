"""AreaD8's tile-contraction path with the clean tiles counted by pointer doubling (ad8_tile_fast_kernel) and the others redone by the Kahn sweep
(ad8_tile_local_kernel over the redo list): bit for bit against the restatement with contamination checking on and off, by default and with
TDX_AD8_LOCAL=kahn (every tile to the Kahn sweep), and the number of redone tiles (tdx_context_ad8_tile_counters) against a numpy predicate of "clean"
evaluated on the same p per 64 x 64 tile - all 64 rows in the raster, the tile and the ring around it inside the raster, every code there 1 .. 8, no
in-tile cycle (ad8_tiles.clean_tiles, which walks every in-tile path step by step) - so that the fast kernel is neither silently unused nor used where it
must not be.  A partial last tile row is not clean, whatever lies below it.

Besides directions derived from a DEM - smooth: short paths, low fan-in - the file holds the kernels to the hand-built tiles of tests/ad8_tiles.py (the
builders are checked on their own, without a GPU, by tests/test_ad8_tiles_model.py): longest in-tile paths on both sides of every power of two, fan-in 7,
every ring cell an entry (the second slot of the lanes 0 .. 3 and the ring corners among them, all at once and each alone), corner exits, rough acyclic
fields at the x edge, cyclic tiles of every kind, and strips cut on tile edges with the per-rank counts."""
import ctypes as C

import numpy as np
import pytest

import ad8_tiles as T
from ad8_tiles import clean_tiles as _clean_tiles
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
    assert T.tile_walk(p, 3 * TS, 3 * TS)[0] and not T.tile_walk(p, 2 * TS, 3 * TS)[0]
    clean = _clean_tiles(p)
    assert clean == {(2, 1), (2, 3), (3, 2)}
    _check(ctx, oracle, monkeypatch, p, clean, "quirks")


def test_three_strips(ctx, oracle, monkeypatch):
    """Strip heights 133, 133, 134: no multiple of 64, the ring rows of a strip's first and last tile rows come from the halo.  The fast / redone counts of strips are asserted by test_strips_* below."""
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


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# hand-built tiles (tests/ad8_tiles.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
INTERIOR_320 = {(y, x) for y in (1, 2, 3) for x in (1, 2, 3)}
# 2^k - 1, 2^k, 2^k + 1 hops, nine tiles per raster (the last raster repeats some)
CHAIN_L = (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4094, 4095)
CHAIN_SETS = (CHAIN_L[0:9], CHAIN_L[9:18], CHAIN_L[18:20] + (63, 4095, 64, 2048, 2047, 4094, 1024))


@pytest.mark.parametrize("Ls", CHAIN_SETS, ids=lambda Ls: f"L{Ls[0]}-{Ls[8]}")
def test_path_lengths_round_boundaries(Ls, ctx, oracle, monkeypatch):
    """After round k the doubling has counted the cells less than 2^(k + 1) hops upstream: a path of 2^k - 1 hops is done one round before a path of 2^k.  A
    liveness vote or a pointer generation that is off by one shows on one side of a power of two.  A second run lowers the big-cell threshold so that cells of fast
    tiles go through the exact re-evaluation (phase D) via the per-cell word."""
    p = T.chain_raster(Ls)
    for i, L in enumerate(Ls):
        assert T.tile_walk(p, (1 + i // 3) * TS, (1 + i % 3) * TS) == (False, L)
    clean = _clean_tiles(p)
    assert clean == INTERIOR_320
    _check(ctx, oracle, monkeypatch, p, clean, f"chain tiles {Ls}")
    monkeypatch.setenv("TDX_AD8_BIG_THRESHOLD", "40")
    _check(ctx, oracle, monkeypatch, p, clean, f"chain tiles {Ls}, big cells from 40")


def test_fan_in_seven(ctx, oracle, monkeypatch):
    """Seven in-tile contributors, the acyclic maximum, at every third cell: the LDS atomics of a round add seven values to one word."""
    p = T.fan7((320, 320))
    clean = _clean_tiles(p)
    assert clean == INTERIOR_320
    assert all(T.in_tile_fan_in(p, y * TS, x * TS).max() == 7 for y, x in clean)
    _check(ctx, oracle, monkeypatch, p, clean, "fan-in 7")
    monkeypatch.setenv("TDX_AD8_BIG_THRESHOLD", "40")
    _check(ctx, oracle, monkeypatch, p, clean, "fan-in 7, big cells from 40")


@pytest.mark.parametrize("n", [192, 320])
def test_every_ring_cell_an_entry(n, ctx, oracle, monkeypatch):
    """259 of the 260 ring cells of the centre tile enter it at once, and over the three exits every ring cell does - the cells 256 .. 259 of ring_cell() order, each
    lane's second entry, and the four corners included.  At 192 the entries come out of redone tiles, at 320 out of fast ones."""
    o = (n // TS // 2) * TS
    union = set()
    for ex in T.RING_EXITS:
        p = T.ring_entries(ex, n)
        union |= T.ring_entry_cells(p, o, o)
        clean = _clean_tiles(p)
        assert clean == ({(1, 1)} if n == 192 else INTERIOR_320)
        _check(ctx, oracle, monkeypatch, p, clean, f"ring entries, exit {ex}, {n}")
        a = ctx.aread8(p, -32768, contcheck=False)
        ey, ex_, code = ex
        assert a[o + ey, o + ex_] >= TS * TS + 259, "the exit cell: its tile and at least the ring"
    assert union == set(range(260))


def test_lone_ring_entries(ctx, oracle, monkeypatch):
    """One entering crossing per tile: from each ring corner and from each of the four second-slot ring cells."""
    for j in (0, TS + 1, TS + 2, 2 * TS + 3, 256, 257, 258, 259):
        p = T.lone_entry(j)
        assert T.ring_entry_cells(p, TS, TS) == {j}
        clean = _clean_tiles(p)
        assert clean == {(1, 1)}
        _check(ctx, oracle, monkeypatch, p, clean, f"lone entry from ring cell {j}")


def test_corner_exits(ctx, oracle, monkeypatch):
    p = T.corner_exits()
    clean = _clean_tiles(p)
    assert clean == {(y, x) for y in (1, 2, 3, 4) for x in (1, 2, 3, 4)}
    _check(ctx, oracle, monkeypatch, p, clean, "corner exits")


@pytest.mark.parametrize("side", sorted(T.SIDES))
@pytest.mark.parametrize("n", [320, 193, 192])
def test_halfplane_fields(n, side, ctx, oracle, monkeypatch):
    """Rough acyclic fields.  With 193 rows and columns the tile at 128 .. 191 is the last that is clean: x0 + TS == nx - 1, its window ends on the raster's last
    column and row; with 192 it is the first that is not (x0 + TS == nx), and only the tile at 64 is."""
    p = T.halfplane((n, n), side, 100 + n)
    clean = _clean_tiles(p)
    assert clean == {320: INTERIOR_320, 193: {(1, 1), (1, 2), (2, 1), (2, 2)}, 192: {(1, 1)}}[n] and len(clean) > 0
    _check(ctx, oracle, monkeypatch, p, clean, f"halfplane {side} {n}")
    if n == 320:
        monkeypatch.setenv("TDX_AD8_BIG_THRESHOLD", "40")
        _check(ctx, oracle, monkeypatch, p, clean, f"halfplane {side} {n}, big cells from 40")


def test_uniform_field_redoes_every_tile(ctx, oracle, monkeypatch):
    """Every interior tile holds cycles: all of them reach the redo list, through the round cap."""
    p = T.uniform((320, 320), 5)
    clean = _clean_tiles(p)
    assert len(clean) == 0
    _check(ctx, oracle, monkeypatch, p, clean, "uniform")


def test_checkerboard_of_fast_and_redone_tiles(ctx, oracle, monkeypatch):
    """Acyclic and cyclic tiles side by side: crossings of dead nodes enter fast tiles, and fast tiles drain into redone ones."""
    p = T.checkerboard(5)
    clean = _clean_tiles(p)
    assert clean == {(1, 1), (1, 3), (2, 2), (3, 1), (3, 3)}
    _check(ctx, oracle, monkeypatch, p, clean, "checkerboard")


def test_cycle_across_two_tiles(ctx, oracle, monkeypatch):
    """Neither tile holds a cycle of its own: both are finished by the fast kernel, and the forest leaves exactly the loop's cells unevaluated."""
    p, loop = T.cross_tile_cycle()
    clean = _clean_tiles(p)
    assert clean == {(1, 1), (1, 2), (1, 3)}
    _check(ctx, oracle, monkeypatch, p, clean, "cross-tile cycle")
    a = ctx.aread8(p, -32768, contcheck=False)
    assert ((a == -1.0) == loop).all() and loop.sum() == 160
    assert (ctx.aread8(p, -32768, contcheck=True)[loop] == -1.0).all()


@pytest.mark.parametrize("box", [(8, 4, 48, 56), (0, 0, 64, 64)], ids=["box", "whole-tile"])
def test_long_cycle_with_feeders(box, ctx, oracle, monkeypatch):
    """A cycle of 2688 (4096) cells with trees above it, entered from the left ring column; no pointer of the tile ever dies, the round cap sends it to the redo list
    after the entry walks ran into their bound."""
    p, tour = T.long_cycle(box)
    clean = _clean_tiles(p)
    assert len(clean) == 0 and T.tile_walk(p, TS, TS) == (True, 0)
    _check(ctx, oracle, monkeypatch, p, clean, f"long cycle {box}")
    a = ctx.aread8(p, -32768, contcheck=False)
    assert ((a == -1.0) == tour).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# strips: per-rank counts
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_strips(oracle, monkeypatch, p, parts, name):
    """p cut into the row strips `parts`, one rank each: the concatenated raster bit for bit against the restatement, and every rank's (fast, redone) against
    clean_tiles(p, rows=its rows), by default and with every tile to the Kahn sweep, contamination checking on and off.  Returns the ranks' clean sets."""
    from taudem_amd.distributed import StripGroup, StripPipeline
    import torch

    ny, nx = p.shape
    assert parts[0][0] == 0 and parts[-1][1] == ny and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
    ref = {cc: oracle.aread8(p, -32768, contcheck=cc) for cc in (True, False)}
    clean = [_clean_tiles(p, rows=r) for r in parts]
    ntiles = [-(-(y1 - y0) // TS) * -(-nx // TS) for y0, y1 in parts]
    p_t = torch.from_numpy(p)
    for mode in ("default", "kahn"):
        if mode == "kahn":
            monkeypatch.setenv("TDX_AD8_LOCAL", "kahn")
        else:
            monkeypatch.delenv("TDX_AD8_LOCAL", raising=False)
        with StripGroup(len(parts), nx) as grp:
            def rank_main(r, c, comm):
                y0, y1 = parts[r]
                pipe = StripPipeline(c, comm, nx, y1 - y0)
                pp = pipe.empty(torch.int16)
                pp[1:y1 - y0 + 1].copy_(p_t[y0:y1])
                out = {}
                for cc in (True, False):
                    a, _ = pipe.aread8(pp, -32768, contcheck=cc)
                    torch.cuda.synchronize()
                    out[cc] = (a[1:y1 - y0 + 1].cpu().numpy(), _counters(c))
                return out
            res = grp.run(rank_main)
        monkeypatch.delenv("TDX_AD8_LOCAL", raising=False)
        for cc in (True, False):
            got = np.concatenate([r[cc][0] for r in res])
            assert bits_equal(got, ref[cc]), describe_diff(got, ref[cc], f"{name}: strips {parts}, {mode}, contcheck={cc}")
            counts = [r[cc][1] for r in res]
            want = [(0, n) for n in ntiles] if mode == "kahn" else [(len(c), n - len(c)) for c, n in zip(clean, ntiles)]
            assert counts == want, f"{name}: fast / redone tiles per rank, strips {parts}, {mode}, contcheck={cc}"
    return clean


def _strip_field(oracle, kind, shape):
    if kind == "dem":
        return _p_field(oracle, shape, 31)
    if kind == "snake":      # chain_tile(4095) in the tile rows 65 .. 128 (64 .. 127 of the 256-row raster): it drains south, out of a one-tile-row strip
        p = np.full(shape, T.E, dtype=np.int16)
        y0 = 65 if shape[0] == 322 else 64
        p[y0:y0 + TS, TS:2 * TS] = T.chain_tile(4095)
        return p
    return T.halfplane(shape, kind, 7)


PARTS_322 = [(0, 65), (65, 129), (129, 257), (257, 322)]


@pytest.mark.parametrize("kind", ["south", "north", "dem", "snake"])
def test_strips_cut_on_tile_edges(kind, oracle, monkeypatch):
    """322 x 193 in strips of 65, 64, 128 and 65 rows: the second strip is exactly one tile row - its clean tiles leave through the halo rows above (NEXT_REMOTE_UP)
    and below (NEXT_REMOTE_DOWN, which needs a whole last tile row) - the third two tile rows, and the outer halo rows of the first and the last are nodata."""
    p = _strip_field(oracle, kind, (322, 193))
    clean = _check_strips(oracle, monkeypatch, p, PARTS_322, kind)
    if kind != "dem":
        assert clean == [set(), {(0, 1), (0, 2)}, {(0, 1), (0, 2), (1, 1), (1, 2)}, {(0, 1), (0, 2)}]
    assert len(clean[1]) > 0 and len(clean[2]) > 0
    if kind == "snake":
        assert T.tile_walk(p, 65, TS) == (False, 4095) and p[65 + TS - 1, TS] == T.S, "the path's last cell, in the strip's last row, flows south into the next rank"


@pytest.mark.parametrize("kind", ["south", "north", "dem", "snake"])
def test_strips_of_one_tile_row(kind, oracle, monkeypatch):
    """256 x 193 in four strips of 64 rows: every clean tile's ring rows are halo rows."""
    p = _strip_field(oracle, kind, (256, 193))
    parts = [(0, 64), (64, 128), (128, 192), (192, 256)]
    clean = _check_strips(oracle, monkeypatch, p, parts, kind)
    if kind != "dem":
        assert clean == [set(), {(0, 1), (0, 2)}, {(0, 1), (0, 2)}, set()]
    assert len(clean[1]) > 0 and len(clean[2]) > 0
    if kind == "snake":
        assert T.tile_walk(p, TS, TS) == (False, 4095) and p[2 * TS - 1, TS] == T.S


def test_strips_corner_exits_across_the_cuts(oracle, monkeypatch):
    """The diagonal exits of the tiles (1, *) cross the cuts at the rows 64 and 128, those of the tiles (3, *) the cut at 256 and, inside a rank, the row 192."""
    p = T.corner_exits()
    clean = _check_strips(oracle, monkeypatch, p, [(0, 64), (64, 128), (128, 256), (256, 384)], "corner exits")
    row = {(0, x) for x in (1, 2, 3, 4)}
    assert clean == [set(), row, row | {(1, x) for x in (1, 2, 3, 4)}, row]


def test_single_strip_form(ctx, oracle, monkeypatch):
    """StripPipeline without a communicator: both halo rows are nodata, so the first and the last tile row are not clean."""
    from taudem_amd.distributed import StripPipeline
    import torch

    ny = nx = 192
    p = T.halfplane((ny, nx), "south", 9)
    clean = _clean_tiles(p, rows=(0, ny))
    assert clean == {(1, 1)}
    pipe = StripPipeline(ctx, None, nx, ny)
    pp = pipe.empty(torch.int16)
    pp[1:ny + 1].copy_(torch.from_numpy(p))
    for cc in (True, False):
        ref = oracle.aread8(p, -32768, contcheck=cc)
        for mode, want in (("default", (1, 8)), ("kahn", (0, 9))):
            if mode == "kahn":
                monkeypatch.setenv("TDX_AD8_LOCAL", "kahn")
            a, _ = pipe.aread8(pp, -32768, contcheck=cc)
            torch.cuda.synchronize()
            got = a[1:ny + 1].cpu().numpy()
            monkeypatch.delenv("TDX_AD8_LOCAL", raising=False)
            assert bits_equal(got, ref), describe_diff(got, ref, f"single strip, {mode}, contcheck={cc}")
            assert _counters(ctx) == want, f"single strip, {mode}"


@pytest.mark.parametrize("seed", range(8))
def test_strips_random_aligned_cuts(seed, oracle, monkeypatch):
    """1024 x 260 in 2 .. 6 strips whose heights are multiples of 64, the cuts and the field's side drawn per seed."""
    rng = np.random.default_rng(1000 + seed)
    side = sorted(T.SIDES)[int(rng.integers(0, 4))]
    size = int(rng.integers(2, 7))
    cuts = sorted(int(c) * TS for c in rng.choice(np.arange(1, 16), size=size - 1, replace=False))
    parts = list(zip([0] + cuts, cuts + [1024]))
    p = T.halfplane((1024, 260), side, 2000 + seed)
    clean = _check_strips(oracle, monkeypatch, p, parts, f"seed {seed}, {side}")
    assert sum(len(c) for c in clean) == 3 * (16 - 2), "every tile row but the raster's first and last, three tile columns of the five"
