"""The hand-built direction fields of tests/ad8_tiles.py are what they claim to be - judged by the plain walk of the helper, by the restatement, and by the model of
ad8_tile_fast_kernel's schedule (scripts/sim/ad8_doubling.c) - before tests/test_gpu_ad8_doubling.py holds the kernels to them.  No GPU."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ad8_tiles as T

TS = T.TS
# longest in-tile paths of 2^k - 1, 2^k and 2^k + 1 hops: the doubling must stop after exactly ceil(log2(L + 1)) rounds
CHAIN_L = (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4094, 4095)


def _centre(tile):
    p = np.full((192, 192), T.E, dtype=np.int16)
    p[TS:2 * TS, TS:2 * TS] = tile
    return p


def _interior(p):
    ty, tx = T.tiles_of(*p.shape)
    return [(y, x) for y in range(1, ty - 1) for x in range(1, tx - 1)]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ad8_tiles")
    exe = tmp / "ad8_doubling"
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "sim", "ad8_doubling.c")
    subprocess.run(["gcc", "-O2", "-w", "-o", str(exe), src], check=True)

    def run(p, name):
        raw = tmp / name
        np.ascontiguousarray(p, dtype=np.int16).tofile(raw)
        out = subprocess.run([str(exe), str(p.shape[0]), str(raw)], check=True, capture_output=True, text=True).stdout
        m = re.search(r"tiles (\d+): clean (\d+), cyclic (\d+), mismatching (\d+); rounds per tile ([\d.]+), at most (\d+)", out)
        assert m, out
        return {"tiles": int(m[1]), "clean": int(m[2]), "cyclic": int(m[3]), "mismatching": int(m[4]), "max_rounds": int(m[6])}
    return run


def test_chain_tiles_have_the_path_length_asked_for(oracle, model):
    """The model counts a round while a pointer is live before it, which is the formula: a path of L hops is done after ceil(log2(L + 1)) rounds (6 for 63, 7 for 64 and
    65, ... 12 for 2048 .. 4095), asserted for every L."""
    rounds = {}
    for L in CHAIN_L:
        p = _centre(T.chain_tile(L))
        assert T.tile_walk(p, TS, TS) == (False, L)
        assert T.clean_tiles(p) == {(1, 1)}
        a = oracle.aread8(p, -32768, contcheck=False)
        assert (a >= 1.0).all(), f"L = {L}: the restatement evaluates every cell"
        r = model(p, f"chain{L}.bin")
        assert (r["tiles"], r["clean"], r["cyclic"], r["mismatching"]) == (9, 1, 0, 0), f"L = {L}: {r}"
        rounds[L] = r["max_rounds"]
        assert r["max_rounds"] == math.ceil(math.log2(L + 1)), f"L = {L}: {r}"
    print("doubling rounds of the model per L:", rounds)
    assert rounds[4095] == 12


@pytest.mark.parametrize("side", sorted(T.SIDES))
def test_halfplane_fields_are_acyclic(side, oracle):
    p = T.halfplane((320, 320), side, 11)
    assert set(np.unique(p)) == set(T.SIDES[side])
    assert not any(T.tile_walk(p, y * TS, x * TS)[0] for y, x in _interior(p))
    assert T.clean_tiles(p) == set(_interior(p)) and len(_interior(p)) == 9
    assert (oracle.aread8(p, -32768, contcheck=False) >= 1.0).all()
    fan = max(int(T.in_tile_fan_in(p, y * TS, x * TS).max()) for y, x in _interior(p))
    assert fan >= 3, "rough: several cells drain to one"


def test_halfplane_exits_leave_through_sides_and_corners():
    """An 'east' tile is left through its right column, its bottom row, its top row (north-east) and its two right corners diagonally."""
    p = T.halfplane((320, 320), "east", 11)
    t = p[TS:2 * TS, TS:2 * TS]
    assert (t[:, -1] == T.E).any() and (t[-1, :] == T.S).any() and (t[0, :] == T.NE).any()
    assert any(p[y * TS, (x + 1) * TS - 1] == T.NE for y, x in _interior(p)) and any(p[(y + 1) * TS - 1, (x + 1) * TS - 1] == T.SE for y, x in _interior(p))


def test_uniform_field_is_cyclic_everywhere(oracle):
    p = T.uniform((320, 320), 5)
    assert all(T.tile_walk(p, y * TS, x * TS)[0] for y, x in _interior(p))
    assert T.clean_tiles(p) == set()
    a = oracle.aread8(p, -32768, contcheck=False)
    share = float((a == -1.0).mean())
    assert 0.05 < share < 1.0, f"{share:.3f} of the cells lie on or below a cycle"


def test_checkerboard_keeps_the_halfplane_tiles_clean():
    assert T.clean_tiles(T.checkerboard(5)) == {(1, 1), (1, 3), (2, 2), (3, 1), (3, 3)}


def test_cross_tile_cycle(oracle):
    p, loop = T.cross_tile_cycle()
    assert loop.sum() == 160
    assert not T.tile_walk(p, TS, TS)[0] and not T.tile_walk(p, TS, 2 * TS)[0]
    assert T.clean_tiles(p) == {(1, 1), (1, 2), (1, 3)}
    a = oracle.aread8(p, -32768, contcheck=False)
    assert ((a == -1.0) == loop).all(), "exactly the loop's cells are left unevaluated"
    assert (oracle.aread8(p, -32768, contcheck=True)[loop] == -1.0).all()


@pytest.mark.parametrize("box", [(8, 4, 48, 56), (0, 0, 64, 64)])
def test_long_cycle(box, oracle):
    p, tour = T.long_cycle(box)
    assert tour.sum() == box[2] * box[3]
    cyclic, longest = T.tile_walk(p, TS, TS)
    assert cyclic and longest == 0, "no walker of the tile ever comes to an end: every pointer is on or above the cycle"
    assert T.clean_tiles(p) == set()
    assert len(T.ring_entry_cells(p, TS, TS)) == TS, "the left ring column flows into the tile"
    a = oracle.aread8(p, -32768, contcheck=False)
    assert ((a == -1.0) == tour).all()
    # the tour is one cycle: following it from its first cell comes back after exactly h * w steps and not before
    y, x, n = TS + box[0], TS + box[1], 0
    while True:
        c = int(p[y, x])
        y, x, n = y + int(T.D2[c]), x + int(T.D1[c]), n + 1
        if (y, x) == (TS + box[0], TS + box[1]) or n > TS * TS:
            break
    assert n == box[2] * box[3]


def test_ring_entries_cover_the_whole_ring(oracle):
    order = T.ring_order()
    assert len(order) == 260 and len(set(order)) == 260
    assert order[256:] == [(60, TS), (61, TS), (62, TS), (63, TS)], "the second slot of the lanes 0 .. 3"
    union = set()
    for n in (192, 320):
        o = (n // TS // 2) * TS
        for ex in T.RING_EXITS:
            p = T.ring_entries(ex, n)
            ent = T.ring_entry_cells(p, o, o)
            assert len(ent) == 259, "every ring cell but the one the exit drains to"
            assert T.tile_walk(p, o, o) == (False, 63)
            assert (oracle.aread8(p, -32768, contcheck=False) >= 1.0).all(), "acyclic as a whole"
            assert len(T.clean_tiles(p)) == (1 if n == 192 else 9)
            union |= ent
    assert union == set(range(260))
    corners = {0, TS + 1, TS + 2, 2 * TS + 3}
    assert [order[j] for j in sorted(corners)] == [(-1, -1), (-1, TS), (TS, -1), (TS, TS)]
    assert corners | {256, 257, 258, 259} <= T.ring_entry_cells(T.ring_entries(T.RING_EXITS[2]), TS, TS), "one raster has all corners and the whole second slot at once"


def test_lone_entries(oracle):
    for j in (0, TS + 1, TS + 2, 2 * TS + 3, 256, 257, 258, 259):
        p = T.lone_entry(j)
        assert T.ring_entry_cells(p, TS, TS) == {j}
        assert T.clean_tiles(p) == {(1, 1)}
        assert (oracle.aread8(p, -32768, contcheck=False) >= 1.0).all()


def test_fan7_reaches_the_acyclic_maximum(oracle):
    p = T.fan7((320, 320))
    assert T.clean_tiles(p) == set(_interior(p))
    for y, x in _interior(p):
        assert T.in_tile_fan_in(p, y * TS, x * TS).max() == 7
    assert (oracle.aread8(p, -32768, contcheck=False) >= 1.0).all()


def test_corner_exits(oracle):
    p = T.corner_exits()
    assert T.clean_tiles(p) == set(_interior(p)) and len(_interior(p)) == 16
    assert (oracle.aread8(p, -32768, contcheck=False) >= 1.0).all()
    for ty in (1, 3):
        for tx in (1, 3):
            y0, x0 = ty * TS, tx * TS
            assert [int(p[y0, x0]), int(p[y0, x0 + 63]), int(p[y0 + 63, x0]), int(p[y0 + 63, x0 + 63])] == [T.NW, T.NE, T.SW, T.SE]


def test_strip_rule():
    """A strip's tiles are anchored at its first row; its first tile row is clean where the row above exists, its last where it is whole and the row below exists.  With
    193 columns the tile column at 128 is the last that is clean (its window ends on column 192, the raster's last), with 192 the one at 64."""
    p = T.halfplane((322, 193), "south", 3)
    parts = [(0, 65), (65, 129), (129, 257), (257, 322)]
    assert [sorted(T.clean_tiles(p, rows=r)) for r in parts] == [[], [(0, 1), (0, 2)], [(0, 1), (0, 2), (1, 1), (1, 2)], [(0, 1), (0, 2)]]
    assert T.clean_tiles(p, rows=(0, 322)) == T.clean_tiles(p)
    q = T.halfplane((192, 192), "north", 3)
    assert T.clean_tiles(q, rows=(0, 192)) == {(1, 1)}
    assert T.clean_tiles(q, rows=(64, 128)) == {(0, 1)} and T.clean_tiles(q, rows=(128, 192)) == set()
