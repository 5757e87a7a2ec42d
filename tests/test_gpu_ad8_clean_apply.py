"""AreaD8's clean tiles without a staged direction window: ad8_tile_fast_kernel reads the codes into registers, takes the exit cell of every entering crossing out
of the pointer doubling (the ROOT of the entry cell - no entry walks) and hands each cell's code to the apply pass in the per-cell word, which
ad8_tile_apply_fast_kernel turns into ad8 without reading p's tile interior; ad8_tile_apply_kernel serves the redo list.

Everything bit for bit against the restatement, contamination checking on and off, in three modes - default, TDX_AD8_LOCAL=kahn (no fast kernel, no marked word),
TDX_AD8_APPLY=full (fast kernel, plain words, the staged apply pass on every tile) - with the fast / redone tile counts of every call against ad8_tiles.clean_tiles.
Every raster's clean and non-clean tiles are asserted on the CPU first: no case runs on something other than what it is about."""
import ctypes as C

import numpy as np
import pytest

import ad8_tiles as T
from ad8_tiles import clean_tiles as _clean_tiles
from conftest import bits_equal, describe_diff

pytestmark = pytest.mark.gpu
TS = 64
MODES = (("default", {}), ("kahn", {"TDX_AD8_LOCAL": "kahn"}), ("apply-full", {"TDX_AD8_APPLY": "full"}))
INTERIOR_320 = {(y, x) for y in (1, 2, 3) for x in (1, 2, 3)}


def _set_mode(monkeypatch, env):
    for k in ("TDX_AD8_LOCAL", "TDX_AD8_APPLY"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _counters(ctx):
    from taudem_amd import _lib

    fast, redone = C.c_int64(), C.c_int64()
    _lib.load().tdx_context_ad8_tile_counters(ctx._h, C.byref(fast), C.byref(redone))
    return fast.value, redone.value


def _check(ctx, oracle, monkeypatch, p, clean, name):
    """Returns the default mode's ad8 for contcheck off / on."""
    ntiles = -(-p.shape[0] // TS) * -(-p.shape[1] // TS)
    out = {}
    for cc in (True, False):
        a_o = oracle.aread8(p, -32768, contcheck=cc)
        for mode, env in MODES:
            _set_mode(monkeypatch, env)
            a = ctx.aread8(p, -32768, contcheck=cc)
            counts = _counters(ctx)
            _set_mode(monkeypatch, {})
            assert bits_equal(a, a_o), describe_diff(a, a_o, f"{name}: {mode}, contcheck={cc}")
            assert counts == ((0, ntiles) if mode == "kahn" else (len(clean), ntiles - len(clean))), f"{name}: fast / redone tiles, {mode}"
            if mode == "default":
                out[cc] = a
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# roots: the exit cell of an entering crossing out of the doubling
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _entry_path_tile(h):
    """A tile whose cell next to the ring's left column - (63, 0) for h < 63, (0, 0) otherwise - lies exactly h hops above the exit of its path: the last row runs
    east for h cells and leaves south (h = 0: the entry cell is itself the exit), or ad8_tiles.chain_tile(h).  Returns (tile, entry row)."""
    if h >= 63:
        return T.chain_tile(h), 0
    t = np.full((TS, TS), T.S, dtype=np.int16)
    t[TS - 1, :h] = T.E
    return t, TS - 1


def _hops_to_exit(p, y0, x0, ly, lx):
    tgt = T.in_tile_targets(p, y0, x0)
    cur, hops = ly * TS + lx, 0
    while tgt[cur] >= 0:
        cur, hops = int(tgt[cur]), hops + 1
        assert hops < TS * TS
    return hops, divmod(cur, TS)


# 0, 1 and 2 hops, then 2^k - 1, 2^k, 2^k + 1 for k = 1 .. 11 (a pointer of 2^k hops dies one round after one of 2^k - 1)
ROOT_HOPS = sorted({0, 1, 2} | {2 ** k + d for k in range(1, 12) for d in (-1, 0, 1)})
ROOT_SETS = [tuple(ROOT_HOPS[i:i + 9]) for i in range(0, len(ROOT_HOPS), 9)]
ROOT_SETS[-1] = ROOT_SETS[-1] + tuple(ROOT_HOPS[:9 - len(ROOT_SETS[-1])])
assert len(ROOT_HOPS) == 33 and all(len(s) == 9 for s in ROOT_SETS) and set().union(*ROOT_SETS) == set(ROOT_HOPS)


@pytest.mark.parametrize("hops", ROOT_SETS, ids=lambda s: f"h{s[0]}-{s[8]}")
def test_entry_paths_of_given_length(hops, ctx, oracle, monkeypatch):
    """320 x 448, everything flows east, so every cell of a tile's first column is entered from the ring; nine interior tiles - the tile columns 1, 3 and 5, plain
    eastward tiles between them - hold an entry path of exactly the nine hop counts given.  A root taken one round early or late, or from the wrong pointer
    generation, sends the crossing to another exit cell: next(node) of the forest is wrong and the counts downstream differ."""
    p = np.full((320, 448), T.E, dtype=np.int16)
    for i, h in enumerate(hops):
        y0, x0 = (1 + i // 3) * TS, (1 + 2 * (i % 3)) * TS
        t, row = _entry_path_tile(h)
        p[y0:y0 + TS, x0:x0 + TS] = t
        got, (ey, ex) = _hops_to_exit(p, y0, x0, row, 0)
        assert got == h and p[y0 + row, x0 - 1] == T.E, "the ring cell west of the entry cell flows into it, and the entry cell lies h hops above its exit"
        assert not (0 <= ey + T.D2[p[y0 + ey, x0 + ex]] < TS and 0 <= ex + T.D1[p[y0 + ey, x0 + ex]] < TS)
    clean = _clean_tiles(p)
    assert clean == {(y, x) for y in (1, 2, 3) for x in (1, 2, 3, 4, 5)}
    _check(ctx, oracle, monkeypatch, p, clean, f"entry paths {hops}")


@pytest.mark.parametrize("n", [192, 320])
def test_all_ring_cells_enter_and_share_one_exit(n, ctx, oracle, monkeypatch):
    """259 of the 260 ring cells enter the centre tile at once and all end at ONE exit cell (its in-degree in the forest: 259), over the three exits every ring cell
    does; at 320 the ring cells belong to fast tiles, at 192 to redone ones."""
    o = (n // TS // 2) * TS
    union = set()
    for ex in T.RING_EXITS:
        p = T.ring_entries(ex, n)
        entries = T.ring_entry_cells(p, o, o)
        assert len(entries) == 259
        union |= entries
        ey, ex_, code = ex
        roots = set()
        for j in entries:
            hy, hx = T.ring_order()[j]
            c = int(p[o + hy, o + hx])
            roots.add(_hops_to_exit(p, o, o, hy + T.D2[c], hx + T.D1[c])[1])
        assert roots == {(ey, ex_)}, "every entering crossing ends at the one exit cell"
        clean = _clean_tiles(p)
        assert clean == ({(1, 1)} if n == 192 else INTERIOR_320)
        a = _check(ctx, oracle, monkeypatch, p, clean, f"ring entries, exit {ex}, {n}")
        assert a[False][o + ey, o + ex_] >= TS * TS + 259
    assert union == set(range(260))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the per-cell word: count in bits 0 .. 12, code in bits 13 .. 16
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _snake_raster():
    p = np.full((192, 192), T.E, dtype=np.int16)
    p[TS:2 * TS, TS:2 * TS] = T.chain_tile(4095)
    return p


@pytest.mark.parametrize("threshold", [None, "40"], ids=["exact", "big-from-40"])
def test_count_4096_next_to_the_code_field(threshold, ctx, oracle, monkeypatch):
    """The 4 095-hop boustrophedon tile: its last cell counts 4096 in the tile - bit 12, the neighbour of the code field.  With big cells from 40 the cells of the
    marked tile go through the exact re-evaluation, sorted by their word: the code must be gone from it."""
    p = _snake_raster()
    assert T.tile_walk(p, TS, TS) == (False, 4095)
    clean = _clean_tiles(p)
    assert clean == {(1, 1)}
    if threshold:
        monkeypatch.setenv("TDX_AD8_BIG_THRESHOLD", threshold)
    a = _check(ctx, oracle, monkeypatch, p, clean, f"snake, threshold {threshold}")
    assert a[False][2 * TS - 1, TS] == 2 * 4096.0, "the 4096 cells of the tile and the 64 x 64 of the tile west of it, which enter row by row"


@pytest.mark.parametrize("threshold", [None, "40"], ids=["exact", "big-from-40"])
@pytest.mark.parametrize("kind", ["chains", "fan7", "halfplane"])
def test_big_cells_out_of_marked_tiles(kind, threshold, ctx, oracle, monkeypatch):
    p = {"chains": lambda: T.chain_raster((63, 64, 65, 511, 512, 513, 4094, 4095, 2048)), "fan7": lambda: T.fan7((320, 320)),
         "halfplane": lambda: T.halfplane((320, 320), "east", 420)}[kind]()
    clean = _clean_tiles(p)
    assert clean == INTERIOR_320
    if threshold:
        monkeypatch.setenv("TDX_AD8_BIG_THRESHOLD", threshold)
    _check(ctx, oracle, monkeypatch, p, clean, f"{kind}, threshold {threshold}")


@pytest.mark.parametrize("threshold", [None, "40"], ids=["exact", "big-from-40"])
@pytest.mark.parametrize("n", [192, 193])
def test_marked_and_plain_words_side_by_side(n, threshold, ctx, oracle, monkeypatch):
    """Three by three whole tiles whose centre tile is clean and whose eight neighbours are not.  At 192 they touch the raster's edge; at 193 the tiles (1, 2), (2, 1)
    and (2, 2) have their window inside the raster (x0 + 64 == nx - 1) and are spoilt by a p == 0 cell, a nodata cell and a 2-cycle in their interiors."""
    p = T.halfplane((n, n), "east", 300 + n)
    if n == 193:
        assert _clean_tiles(p) == {(1, 1), (1, 2), (2, 1), (2, 2)}
        p[1 * TS + 30, 2 * TS + 30] = 0
        p[2 * TS + 30, 1 * TS + 30] = -32768
        p[2 * TS + 30, 2 * TS + 30], p[2 * TS + 30, 2 * TS + 31] = T.E, T.W
        assert T.tile_walk(p, 2 * TS, 2 * TS)[0]
    clean = _clean_tiles(p)
    assert clean == {(1, 1)}
    if threshold:
        monkeypatch.setenv("TDX_AD8_BIG_THRESHOLD", threshold)
    _check(ctx, oracle, monkeypatch, p, clean, f"one clean tile among eight others, {n}, threshold {threshold}")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# contamination and "not evaluated" entering a clean tile
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
OPPOSITE = {T.E: T.W, T.W: T.E, T.N: T.S, T.S: T.N, T.SE: T.NW, T.NW: T.SE, T.NE: T.SW, T.SW: T.NE}
CENTRE = (2, 2)


def _first_in_centre(d):
    """Row / column of the first cell of the centre tile on the line through (160, 160) that advances by d per step."""
    return 160 if d == 0 else (CENTRE[0] * TS if d > 0 else (CENTRE[0] + 1) * TS - 1)


def _flag_field(code, cond):
    """320 x 320, every cell flows by `code`: each flow line starts on the raster's edge, so edge contamination enters every clean tile.  The line through the
    centre cell (160, 160) of the centre tile (2, 2) crosses the tile before it - through a side, or through the corner for the diagonal code.  cond:
      edge   nothing else
      quirk  a p == 0 cell north-west of the line's cell 50 steps above the centre: that cell is never evaluated (the reference counts the p == 0 neighbour in and
             never counts it down), nor is anything below it
      cycle  that cell and the next one of the line form a 2-cycle inside the neighbouring tile: what lies above is never evaluated, the line starts anew below
      never  the line's last cell before the centre tile and its first cell in it form a 2-cycle ACROSS the tile edge: neither tile holds a cycle, the crossing's
             node in the forest never completes, and what flows into the centre tile's cell stays unevaluated
    Returns (p, the neighbouring tile)."""
    dy, dx = int(T.D2[code]), int(T.D1[code])
    p = np.full((320, 320), code, dtype=np.int16)
    qy, qx = 160 - 50 * dy, 160 - 50 * dx
    if cond == "quirk":
        p[qy - 1, qx - 1] = 0
    elif cond == "cycle":
        p[qy + dy, qx + dx] = OPPOSITE[code]
    elif cond == "never":
        vy, vx = _first_in_centre(dy), _first_in_centre(dx)
        assert (vy // TS, vx // TS) == CENTRE and ((vy - dy) // TS, (vx - dx) // TS) != CENTRE
        p[vy, vx] = OPPOSITE[code]
    else:
        assert cond == "edge"
    return p, (CENTRE[0] - dy, CENTRE[1] - dx)


@pytest.mark.parametrize("cond", ["edge", "quirk", "cycle", "never"])
@pytest.mark.parametrize("code", [T.E, T.S, T.W, T.N, T.SE], ids=["from-west", "from-north", "from-east", "from-south", "through-corner"])
def test_flags_enter_a_clean_tile(code, cond, ctx, oracle, monkeypatch):
    p, upstream = _flag_field(code, cond)
    clean = _clean_tiles(p)
    assert CENTRE in clean, "the tile the flags enter is finished by the fast kernels"
    if cond in ("quirk", "cycle"):
        assert upstream not in clean and clean == INTERIOR_320 - {upstream}
    else:
        assert clean == INTERIOR_320
    a = _check(ctx, oracle, monkeypatch, p, clean, f"code {code}, {cond}")
    dy, dx = int(T.D2[code]), int(T.D1[code])
    centre_val = a[False][160, 160]
    if cond == "quirk":
        assert centre_val == -1.0, "not evaluated: the flag went down the line inside the clean tile"
    elif cond == "never":
        vy, vx = _first_in_centre(dy), _first_in_centre(dx)
        assert a[False][vy, vx] == -1.0 and a[False][vy - dy, vx - dx] == -1.0, "the two cells of the cycle across the tile edge"
        assert centre_val == abs(160 - (vy if dy else vx)) or (dy and dx), "the line starts anew behind the centre tile's first cell"
        assert centre_val > 0
    elif cond == "cycle":
        assert centre_val == 49.0 or (dy and dx), "the line starts anew below the cycle: 48 cells above the centre cell (more on the diagonal, which the rows and columns feed)"
        assert centre_val > 0 and a[True][160, 160] == centre_val, "and what starts anew there never saw the raster's edge"
    else:
        assert (a[True][CENTRE[0] * TS:(CENTRE[0] + 1) * TS, CENTRE[1] * TS:(CENTRE[1] + 1) * TS] == -1.0).all(), "every flow line starts on the raster's edge"
        assert centre_val == (161.0 if dy + dx > 0 else 160.0) or (dy and dx), "the cells of the line from the raster's edge to the centre cell"
        assert centre_val > 0


def test_loop_through_two_clean_tiles(ctx, oracle, monkeypatch):
    """A crossing that never delivers with a PATH below it in the clean tile: the 160-cell loop of ad8_tiles.cross_tile_cycle enters each of its two tiles (both
    clean) through one ring cell and leaves it 40 and more cells further on; exactly the loop's cells stay unevaluated."""
    p, loop = T.cross_tile_cycle()
    clean = _clean_tiles(p)
    assert clean == {(1, 1), (1, 2), (1, 3)}
    a = _check(ctx, oracle, monkeypatch, p, clean, "cross-tile loop")
    assert ((a[False] == -1.0) == loop).all() and loop.sum() == 160 and (a[True][loop] == -1.0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# strips
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_strips(oracle, monkeypatch, p, parts, name):
    from taudem_amd.distributed import StripGroup, StripPipeline
    import torch

    ny, nx = p.shape
    assert parts[0][0] == 0 and parts[-1][1] == ny and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
    ref = {cc: oracle.aread8(p, -32768, contcheck=cc) for cc in (True, False)}
    clean = [_clean_tiles(p, rows=r) for r in parts]
    ntiles = [-(-(y1 - y0) // TS) * -(-nx // TS) for y0, y1 in parts]
    p_t = torch.from_numpy(p)
    for mode, env in MODES:
        _set_mode(monkeypatch, env)
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
        _set_mode(monkeypatch, {})
        for cc in (True, False):
            got = np.concatenate([r[cc][0] for r in res])
            assert bits_equal(got, ref[cc]), describe_diff(got, ref[cc], f"{name}: strips {parts}, {mode}, contcheck={cc}")
            counts = [r[cc][1] for r in res]
            want = [(0, n) for n in ntiles] if mode == "kahn" else [(len(c), n - len(c)) for c, n in zip(clean, ntiles)]
            assert counts == want, f"{name}: fast / redone tiles per rank, strips {parts}, {mode}, contcheck={cc}"
    return clean


def _strip_field(kind, shape, first_row):
    if kind == "snake":      # the 4 095-hop tile in the second strip: its last cell, in the strip's last row, flows south into the next rank
        p = np.full(shape, T.E, dtype=np.int16)
        p[first_row:first_row + TS, TS:2 * TS] = T.chain_tile(4095)
        return p
    return T.halfplane(shape, kind, 11)


@pytest.mark.parametrize("kind", ["south", "north", "snake"])
def test_strips_of_one_tile_row(kind, oracle, monkeypatch):
    """320 x 193 in five strips of 64 rows: the first, the middle and the last strips each hold tiles with the window inside the array, every ring row is a halo row,
    exits leave upwards (north) and downwards (south, snake), and the outer halo rows of the first and last strip are nodata."""
    p = _strip_field(kind, (320, 193), TS)
    parts = [(i * TS, (i + 1) * TS) for i in range(5)]
    clean = _check_strips(oracle, monkeypatch, p, parts, kind)
    assert clean == [set(), {(0, 1), (0, 2)}, {(0, 1), (0, 2)}, {(0, 1), (0, 2)}, set()]


@pytest.mark.parametrize("kind", ["south", "north", "snake"])
def test_strips_cut_on_tile_edges(kind, oracle, monkeypatch):
    """322 x 193 as 65 / 64 / 128 / 65 rows: tiles anchored at the rows 65, 129 and 257.  The first and last strips have a whole tile row and a one-row one."""
    p = _strip_field(kind, (322, 193), 65)
    clean = _check_strips(oracle, monkeypatch, p, [(0, 65), (65, 129), (129, 257), (257, 322)], kind)
    assert clean == [set(), {(0, 1), (0, 2)}, {(0, 1), (0, 2), (1, 1), (1, 2)}, {(0, 1), (0, 2)}]


def test_strips_with_clean_tiles_in_first_middle_and_last(oracle, monkeypatch):
    """260 x 193 as 130 / 65 / 65 rows with tiles anchored at 0, 130 and 195: whole tile rows (64 .. 127 in the first strip, 130 .. 193 in the middle one, 195 .. 258
    in the last) whose ring rows are owned rows on one side and halo rows on the other."""
    p = T.halfplane((260, 193), "south", 13)
    clean = _check_strips(oracle, monkeypatch, p, [(0, 130), (130, 195), (195, 260)], "130/65/65")
    assert clean == [{(1, 1), (1, 2)}, {(0, 1), (0, 2)}, {(0, 1), (0, 2)}]


def test_single_strip_form(ctx, oracle, monkeypatch):
    """StripPipeline without a communicator: both halo rows are nodata, the first and the last tile row are not clean."""
    from taudem_amd.distributed import StripPipeline
    import torch

    ny = nx = 192
    p = T.halfplane((ny, nx), "north", 15)
    assert _clean_tiles(p, rows=(0, ny)) == {(1, 1)}
    pipe = StripPipeline(ctx, None, nx, ny)
    pp = pipe.empty(torch.int16)
    pp[1:ny + 1].copy_(torch.from_numpy(p))
    for cc in (True, False):
        ref = oracle.aread8(p, -32768, contcheck=cc)
        for mode, env in MODES:
            _set_mode(monkeypatch, env)
            a, _ = pipe.aread8(pp, -32768, contcheck=cc)
            torch.cuda.synchronize()
            got = a[1:ny + 1].cpu().numpy()
            _set_mode(monkeypatch, {})
            assert bits_equal(got, ref), describe_diff(got, ref, f"single strip, {mode}, contcheck={cc}")
            assert _counters(ctx) == ((0, 9) if mode == "kahn" else (1, 8)), f"single strip, {mode}"


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# TDX_AD8_DEBUG=1: the clocked instantiations of the four tile kernels
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
_DEBUG_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import taudem_amd
with taudem_amd.Context(0) as ctx:
    np.save(sys.argv[3], ctx.aread8(np.load(sys.argv[2]), -32768))
"""
_CLOCK_FIELDS = {"ad8_tile_local": 6, "ad8_tile_fast": 6, "ad8_tile_apply": 4, "ad8_tile_apply_fast": 4}   # (the fast kernel's sixth: rounds per tile)


def test_debug_clocks_in_a_child_process(tmp_path):
    """TDX_AD8_DEBUG is read once per process, so the clocked (<true>) instantiations run in a child process and the baseline in a second one, which never saw the switch.
    192 x 192 draining east: of the 3 x 3 tiles only the middle one is clean, and its left ring column enters it.  Same bits with and without the clocks, one
    "cycles per tile" line per tile kernel, tile counts (redone, clean, redone, clean) as ad8_tiles.clean_tiles gives them, every figure a non-negative number."""
    import os
    import re
    import subprocess
    import sys

    p = np.full((192, 192), T.E, dtype=np.int16)
    clean = _clean_tiles(p)
    assert clean == {(1, 1)} and len(T.ring_entry_cells(p, TS, TS)) >= 1
    redone = 9 - len(clean)
    np.save(tmp_path / "p.npy", p)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {}
    for name, debug in (("plain", False), ("clocked", True)):
        env = {k: v for k, v in os.environ.items() if not k.startswith("TDX_AD8_")}
        if debug:
            env["TDX_AD8_DEBUG"] = "1"
        r = subprocess.run([sys.executable, "-c", _DEBUG_CHILD, root, str(tmp_path / "p.npy"), str(tmp_path / f"{name}.npy")], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, f"{name}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-6000:]}"
        runs[name] = (np.load(tmp_path / f"{name}.npy"), r.stderr)
    assert bits_equal(runs["clocked"][0], runs["plain"][0]), describe_diff(runs["clocked"][0], runs["plain"][0], "TDX_AD8_DEBUG=1 against a process without it")
    assert not any(l.startswith("ad8_tile_") for l in runs["plain"][1].splitlines()), "no clock line without the switch"
    lines = [l for l in runs["clocked"][1].splitlines() if l.startswith("ad8_tile_")]
    print("\n".join(lines))
    want_tiles = {"ad8_tile_local": redone, "ad8_tile_fast": len(clean), "ad8_tile_apply": redone, "ad8_tile_apply_fast": len(clean)}
    for kernel, nfields in _CLOCK_FIELDS.items():
        mine = [l for l in lines if l.startswith(kernel + ":")]
        assert len(mine) == 1, f"exactly one line of {kernel}: {lines}"
        m = re.fullmatch(rf"{kernel}: (\d+) tiles, cycles per tile: (.*)", mine[0])
        assert m, mine[0]
        assert int(m.group(1)) == want_tiles[kernel], mine[0]
        fields = re.split(r"[,;]", m.group(2))
        assert len(fields) == nfields, mine[0]
        for f in fields:
            numbers = [w for w in f.split() if re.fullmatch(r"\d+(\.\d+)?", w)]
            assert len(numbers) == 1 and float(numbers[0]) >= 0.0, f"{mine[0]}: field {f!r}"
    assert len(lines) == 4, lines
