"""Hand-built D8 direction fields for AreaD8's tile contraction, and the plain predicates that say what the kernels must do with them (numpy only; no test file).

A 64 x 64 tile is CLEAN - ad8_tile_fast_kernel must finish it by pointer doubling - when all its rows are owned, the 66 x 66 window around it lies inside the raster, every
code in the window is 1 .. 8 and the flows that stay inside the tile hold no cycle.  tile_walk() decides the last point by following every cell's in-tile pointer one
step at a time: nothing here doubles a pointer, so that the predicate shares no method with the kernel it judges."""
import numpy as np

TS = 64
NODATA = -32768
# direction codes 1 .. 8: 1 = E, 2 = NE, 3 = N, 4 = NW, 5 = W, 6 = SW, 7 = S, 8 = SE (index 0 unused)
D1 = np.array([0, 1, 1, 0, -1, -1, -1, 0, 1])    # column step
D2 = np.array([0, 0, -1, -1, -1, 0, 1, 1, 1])    # row step
E, NE, N, NW, W, SW, S, SE = range(1, 9)
SIDES = {"east": (E, NE, SE, S), "south": (S, SW, SE, W), "west": (W, NW, SW, N), "north": (N, NE, NW, E)}


def in_tile_targets(p, y0, x0):
    """Flat in-tile index of the cell every cell of the tile at (y0, x0) drains to, or -1 where the flow leaves the tile or the code is not 1 .. 8."""
    t = np.asarray(p[y0:y0 + TS, x0:x0 + TS]).astype(np.int64)
    assert t.shape == (TS, TS), "tile_walk is for whole tiles"
    ok = (t >= 1) & (t <= 8)
    c = np.where(ok, t, 0)
    ly, lx = np.mgrid[0:TS, 0:TS]
    vy, vx = ly + D2[c], lx + D1[c]
    ok &= (vy >= 0) & (vy < TS) & (vx >= 0) & (vx < TS)
    return np.where(ok, vy * TS + vx, -1).ravel()


def tile_walk(p, y0, x0):
    """(cyclic, longest_hops) of the 64 x 64 tile at (y0, x0): every cell follows its in-tile pointer for 4096 plain steps.  A walker that is still inside the tile after
    4096 steps has visited a cell twice: the tile holds a cycle.  longest_hops is the largest number of hops after which a walker came to the end of its in-tile path."""
    tgt = in_tile_targets(p, y0, x0)
    cur = np.arange(TS * TS)
    longest = 0
    for step in range(1, TS * TS + 1):
        before = cur.size
        cur = tgt[cur]
        cur = cur[cur >= 0]           # the walkers that made this hop
        if cur.size < before:
            longest = step - 1        # some walker could not: it had made step - 1 hops
        if cur.size == 0:
            return False, longest
    return True, longest


def tiles_of(ny, nx):
    return -(-ny // TS), -(-nx // TS)


def clean_tiles(p, rows=None):
    """The set of (ty, tx) that the fast kernel must finish.  rows = (y0, y1): the tiles of the strip that owns the rows [y0, y1) of p, anchored at row y0; a strip sees
    its neighbours' rows as halo rows and nodata outside the raster, so the window is judged on the whole raster."""
    ny, nx = p.shape
    r0, r1 = (0, ny) if rows is None else rows
    tiles_y, tiles_x = tiles_of(r1 - r0, nx)
    clean = set()
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            y0, x0 = r0 + ty * TS, tx * TS
            if y0 + TS > r1:                                                   # a partial last tile row
                continue
            if y0 < 1 or x0 < 1 or y0 + TS > ny - 1 or x0 + TS > nx - 1:      # the window leaves the raster
                continue
            w = p[y0 - 1:y0 + TS + 1, x0 - 1:x0 + TS + 1]
            if not ((w >= 1) & (w <= 8) & (w != NODATA)).all():
                continue
            if tile_walk(p, y0, x0)[0]:
                continue
            clean.add((ty, tx))
    return clean


def in_tile_fan_in(p, y0, x0):
    """Number of cells of the tile at (y0, x0) that drain to each of its cells, 64 x 64."""
    tgt = in_tile_targets(p, y0, x0)
    return np.bincount(tgt[tgt >= 0], minlength=TS * TS).reshape(TS, TS)


def ring_order():
    """The 260 ring cells of a tile as (hy, hx) relative to its first cell, in the kernels' ring_cell() order: the row above (66), the row below (66), the left column (64),
    the right column (64).  A workgroup has 256 lanes: the cells 256 .. 259, the right column's rows 60 .. 63, are each lane's second entry."""
    return ([(-1, j - 1) for j in range(TS + 2)] + [(TS, j - 1) for j in range(TS + 2)] + [(j, -1) for j in range(TS)] + [(j, TS) for j in range(TS)])


def ring_entry_cells(p, y0, x0):
    """Indices (ring_order()) of the ring cells of the tile at (y0, x0) whose flow enters the tile."""
    out = set()
    for j, (hy, hx) in enumerate(ring_order()):
        c = int(p[y0 + hy, x0 + hx])
        if 1 <= c <= 8 and 0 <= hy + D2[c] < TS and 0 <= hx + D1[c] < TS:
            out.add(j)
    return out


# --------------------------------------------------------------------------------------------------------------------------------------------------------------------
# builders: int16 direction fields
# --------------------------------------------------------------------------------------------------------------------------------------------------------------------
def chain_tile(L):
    """A 64 x 64 tile whose longest in-tile path has exactly L hops, 63 <= L <= 4095: rows 0 .. r - 1 are a full boustrophedon (even rows east, odd rows west, the end
    cell of each row south), row r goes on for j cells and turns south, every other cell of row r and every row below flows south: L = 63 r + j + 62."""
    assert 63 <= L <= 4095
    r = min(63, (L - 63) // 63)
    j = L - 62 - 63 * r
    assert 0 <= r <= 63 and 1 <= j <= 64
    t = np.full((TS, TS), S, dtype=np.int16)
    for ly in range(r):
        t[ly, :] = E if ly % 2 == 0 else W
        t[ly, TS - 1 if ly % 2 == 0 else 0] = S
    if r % 2 == 0:
        t[r, :j - 1] = E
    else:
        t[r, TS - (j - 1):] = W
    return t


def chain_raster(Ls):
    """320 x 320, everything flows east, the nine interior tiles are chain_tile(L) for the nine L given (row by row).  Every chain tile drains south."""
    assert len(Ls) == 9
    p = np.full((320, 320), E, dtype=np.int16)
    for i, L in enumerate(Ls):
        ty, tx = 1 + i // 3, 1 + i % 3
        p[ty * TS:(ty + 1) * TS, tx * TS:(tx + 1) * TS] = chain_tile(L)
    return p


def fan7(shape):
    """A lattice of 3 x 3 blocks: the centre of each block receives seven of its neighbours - all but the eastern one - and flows east, the eastern one flows east into
    the next block's western cell, which flows east into that block's centre.  Acyclic (every path reaches a centre row and goes east), every centre has in-degree 7."""
    block = np.array([[SE, S, SW], [E, E, E], [NE, N, NW]], dtype=np.int16)
    ny, nx = shape
    return np.ascontiguousarray(np.tile(block, (-(-ny // 3), -(-nx // 3)))[:ny, :nx])


def ring_entries(exit, n=192):
    """n x n with the centre tile's ring all entries.  exit = (ly, lx, code): every cell of the centre tile steps towards the cell (ly, lx) on the tile's rim, which leaves
    the tile by `code` (east, south-east, south, north-east or north).  Every ring cell points into the tile - the rows above and below straight down and up, the columns
    straight right and left, the four corners diagonally - except the one ring cell that the exit drains to: pointing in it would close a 2-cycle across the tile edge, so
    it carries the flow on in the exit's direction.  Everything else flows east: the raster is acyclic, the whole tile and all that enters it leave through one cell."""
    ey, ex, code = exit
    assert code in (E, SE, S, NE, N) and not (0 <= ey + D2[code] < TS and 0 <= ex + D1[code] < TS)
    assert n % TS == 0 and (n // TS) % 2 == 1
    o = (n // TS // 2) * TS
    p = np.full((n, n), E, dtype=np.int16)
    step = {(0, 1): E, (-1, 1): NE, (-1, 0): N, (-1, -1): NW, (0, -1): W, (1, -1): SW, (1, 0): S, (1, 1): SE}
    for ly in range(TS):
        for lx in range(TS):
            if (ly, lx) != (ey, ex):
                p[o + ly, o + lx] = step[(int(np.sign(ey - ly)), int(np.sign(ex - lx)))]
    p[o + ey, o + ex] = code
    p[o - 1, o:o + TS] = S
    p[o + TS, o:o + TS] = N
    p[o:o + TS, o - 1] = E
    p[o:o + TS, o + TS] = W
    p[o - 1, o - 1], p[o - 1, o + TS], p[o + TS, o - 1], p[o + TS, o + TS] = SE, SW, NE, NW
    p[o + ey + D2[code], o + ex + D1[code]] = code
    return p


RING_EXITS = ((63, 63, SE), (61, 63, E), (0, 20, N))   # a corner, a second-slot ring cell, the row above (the halo row of a strip cut on the tile edge)


def lone_entry(j):
    """192 x 192 whose centre tile has ONE entering crossing, from ring cell j (ring_order()): the tile flows east (west where j lies in the right column), and everything
    around it flows away from it."""
    o = TS
    p = np.empty((192, 192), dtype=np.int16)
    p[:o, :], p[o + TS:, :] = N, S
    p[:, :o], p[:, o + TS:] = W, E
    p[o:o + TS, o:o + TS] = E
    hy, hx = ring_order()[j]
    if hx == TS and 0 <= hy < TS:          # an entry from the right column: the tile flows west, away from it
        p[o:o + TS, o:o + TS] = W
    p[o + hy, o + hx] = {(-1, -1): SE, (-1, TS): SW, (TS, -1): NE, (TS, TS): NW}.get((hy, hx), S if hy < 0 else N if hy >= TS else E if hx < 0 else W)
    return p


def corner_exits():
    """384 x 384, everything flows east; the four corner cells of the tiles (1, 1), (1, 3), (3, 1), (3, 3) leave diagonally into the diagonal neighbour tile, where the flow
    goes on east.  (Not in every tile: two diagonal neighbours would close 2-cycles through their touching corners.)  Every interior tile is clean."""
    p = np.full((384, 384), E, dtype=np.int16)
    for ty in (1, 3):
        for tx in (1, 3):
            y0, x0 = ty * TS, tx * TS
            p[y0, x0], p[y0, x0 + TS - 1], p[y0 + TS - 1, x0], p[y0 + TS - 1, x0 + TS - 1] = NW, NE, SW, SE
    return p


def halfplane(shape, side, seed):
    """Each code drawn uniformly from four neighbouring directions.  Every step increases a linear functional (east: 2 x + y) - acyclic; rough, fan-in 3 - 4 is common, and
    the exits of a tile go through three sides and two corners."""
    rng = np.random.default_rng(seed)
    return np.array(SIDES[side], dtype=np.int16)[rng.integers(0, 4, size=shape)]


def uniform(shape, seed):
    """Codes uniform in 1 .. 8: some 250 two-cycles in every tile."""
    return np.random.default_rng(seed).integers(1, 9, size=shape).astype(np.int16)


def checkerboard(seed):
    """320 x 320: the tiles with ty + tx even from halfplane('east'), the others uniform."""
    p, u = halfplane((320, 320), "east", seed), uniform((320, 320), seed + 1)
    for ty in range(5):
        for tx in range(5):
            if (ty + tx) % 2:
                p[ty * TS:(ty + 1) * TS, tx * TS:(tx + 1) * TS] = u[ty * TS:(ty + 1) * TS, tx * TS:(tx + 1) * TS]
    return p


CROSS_ROWS, CROSS_COLS = (80, 100), (100, 160)


def cross_tile_cycle():
    """192 x 320, everything flows east, but a rectangular loop (clockwise) runs through the rows 80 .. 100 and the columns 100 .. 160: 160 cells, across the tile edge at
    column 128.  Neither tile holds a cycle of its own.  Returns (p, mask of the loop's cells)."""
    p = np.full((192, 320), E, dtype=np.int16)
    (ya, yb), (xa, xb) = CROSS_ROWS, CROSS_COLS
    p[ya, xa:xb] = E
    p[ya:yb, xb] = S
    p[yb, xa + 1:xb + 1] = W
    p[ya + 1:yb + 1, xa] = N
    loop = np.zeros(p.shape, dtype=bool)
    loop[ya, xa:xb + 1] = loop[yb, xa:xb + 1] = True
    loop[ya:yb + 1, xa] = loop[ya:yb + 1, xb] = True
    return p, loop


def long_cycle(box=(8, 4, 48, 56)):
    """192 x 192, everything flows east; inside the centre tile a closed tour (a comb: the first row east, then a boustrophedon down the other columns, the first column
    back up) through every cell of the box (oy, ox, h, w), and every other cell of the tile flows towards the box: chains and trees that feed the cycle.  The ring cells
    of the left column flow east into the tile and from there into the cycle; nothing leaves the tile.  Returns (p, mask of the tour's cells)."""
    oy, ox, h, w = box
    assert h % 2 == 0 and h >= 2 and w >= 2 and oy >= 0 and ox >= 0 and oy + h <= TS and ox + w <= TS
    t = np.empty((TS, TS), dtype=np.int16)
    t[:oy, :], t[oy + h:, :] = S, N
    t[:, :ox], t[:, ox + w:] = E, W
    b = np.empty((h, w), dtype=np.int16)
    b[0, :] = E
    b[0, w - 1] = S
    for r in range(1, h):
        b[r, 1:] = W if r % 2 else E
        if r < h - 1:
            b[r, 1 if r % 2 else w - 1] = S
    b[1:, 0] = N
    t[oy:oy + h, ox:ox + w] = b
    p = np.full((192, 192), E, dtype=np.int16)
    p[TS:2 * TS, TS:2 * TS] = t
    tour = np.zeros(p.shape, dtype=bool)
    tour[TS + oy:TS + oy + h, TS + ox:TS + ox + w] = True
    return p, tour
