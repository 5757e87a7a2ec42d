"""Lake rasters whose open-water block layout is known (flats.hpp: OPEN WATER).

A lake is a flat at H_FLAT inside a one-cell wall at H_WALL, perched on a tilted ground plane far below, so every lake is on its own.  The flat holds
`nbx` aligned blocks of k x k full 64 x 64 tiles side by side, the one-cell ring around them and `margin` more cells on every side.  What the first
flat iteration of D8FlowDir / DinfFlowDir makes of it is set per lake:

- fall ((E, j), ...): incfall sources.  A notch at H_FLAT in the wall, margin + 1 cells out from ring edge E at position j, with the ground behind it:
  the notch drains, so the flat cells beside it are incfall's level-1 seeds.  With margin 0 these are ring cells j - 1 .. j + 1 of edge E.
- rise ((E, j), ...): incrise sources.  A rock at H_WALL one cell out from ring edge E at position j (margin >= 2, so the wall is farther away):
  ring cells j - 1 .. j + 1 of edge E have a higher neighbour, incrise's level 1, before any other ring cell.
- no fall source (and no nodata shore): the lake does not drain, incfall never reaches it.
- islands ((y, x, h, w), ...): rocks at H_WALL relative to the first block's top-left cell; a tile they touch is not full.
- nodata: the bottom wall's cells become nodata (margin >= 2): the margin row beside them is out of the queue without a direction (incfall's
  level-2 "quirk" seeds).

Ring edges and positions are those of LevelOpT::macro_update: edge 0 the row above, 1 the row below, 2 the column left, 3 the column right, position j
= 0 .. L - 1 from the top-left corner along the edge, L = 64 k nbx + 2 (rows) or 64 k + 2 (columns).

The model half (queue, masks, full tiles, blocks) restates flatk::classify_stream_kernel and flatk::find_blocks_kernel on the CPU, so that a test can say
which blocks a raster holds before it runs a GPU."""
from dataclasses import dataclass

import numpy as np

TS = 64
H_FLAT = np.float32(500.0)
H_WALL = np.float32(600.0)
NODATA = np.float32(-3.0e38)
OUT = ((-1, 0), (1, 0), (0, -1), (0, 1))   # outward step of ring edge E (dy, dx)
# The rasters' ground is rough: a single-cell pit in about one cell of nine makes the first flat queue dense (more than 1/16 of the raster), so that
# DinfFlowDir too takes the streaming classification and with it the blocks (dinfflowdir.hip), not only D8FlowDir
ROUGH = 0.5


@dataclass
class Lake:
    k: int
    tx: int                  # first block's first tile (aligned to k)
    ty: int
    nbx: int = 1
    margin: int = 0
    fall: tuple = ()
    rise: tuple = ()
    islands: tuple = ()
    nodata: bool = False
    blocks: tuple = None     # expected (tx, ty, K) of every block in the lake (default: the nbx blocks)
    clip: bool = False       # the lake runs off the raster's right / bottom edge (into a partial tile)

    def __post_init__(self):
        assert self.tx % self.k == 0 and self.ty % self.k == 0
        assert not self.rise or self.margin >= 2
        assert not self.nodata or self.margin >= 2
        if self.blocks is None:
            self.blocks = tuple((self.tx + i * self.k, self.ty, self.k) for i in range(self.nbx))

    @property
    def origin(self):
        return self.ty * TS, self.tx * TS

    @property
    def size(self):   # (height, width) of the blocks
        return self.k * TS, self.k * TS * self.nbx

    def ring_len(self, E):
        H, W = self.size
        return (W if E < 2 else H) + 2

    def ring_cell(self, E, j):
        (Y0, X0), (H, W) = self.origin, self.size
        assert 0 <= j < self.ring_len(E)
        return ((Y0 - 1, X0 - 1 + j), (Y0 + H, X0 - 1 + j), (Y0 - 1 + j, X0 - 1), (Y0 - 1 + j, X0 + W))[E]

    def ring_cells(self, E):
        return [self.ring_cell(E, j) for j in range(self.ring_len(E))]

    def box(self, grow):   # [y0, y1) x [x0, x1) of the blocks grown by `grow` cells
        (Y0, X0), (H, W) = self.origin, self.size
        return Y0 - grow, Y0 + H + grow, X0 - grow, X0 + W + grow

    def draw(self, z):
        m = self.margin
        wy0, wy1, wx0, wx1 = self.box(m + 2)
        assert wy0 >= 0 and wx0 >= 0 and (self.clip or (wy1 <= z.shape[0] and wx1 <= z.shape[1])), "lake outside the raster"
        z[wy0:wy1, wx0:wx1] = H_WALL
        fy0, fy1, fx0, fx1 = self.box(m + 1)
        z[fy0:fy1, fx0:fx1] = H_FLAT
        Y0, X0 = self.origin
        for (y, x, h, w) in self.islands:
            z[Y0 + y:Y0 + y + h, X0 + x:X0 + x + w] = H_WALL
        if self.nodata:
            z[wy1 - 1, wx0 + 1:wx1 - 1] = NODATA
        for (E, j) in self.fall:
            y, x = self.ring_cell(E, j)
            z[y + (m + 1) * OUT[E][0], x + (m + 1) * OUT[E][1]] = H_FLAT
        for (E, j) in self.rise:
            y, x = self.ring_cell(E, j)
            z[y + OUT[E][0], x + OUT[E][1]] = H_WALL


def ground(shape, rough=0.0, seed=0):
    """a plane that falls towards (0, 0) - no flat, no pit - far below the lakes; rough > 0 adds noise of that height (single-cell pits: flats of one cell
    in nearly every tile)"""
    ny, nx = shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    z = (1.0 + 0.001 * xx + 0.0007 * yy).astype(np.float32)
    if rough:
        z += (np.random.default_rng(seed).random(shape) * rough).astype(np.float32)
    return z


def make_dem(shape, lakes, rough=0.0, seed=0):
    z = ground(shape, rough, seed)
    for lk in lakes:
        lk.draw(z)
    return z


# ---- the model: what the streaming classification and find_blocks_kernel make of a raster (first flat iteration) ----
D1 = (0, 1, 1, 0, -1, -1, -1, 0, 1)    # dx of neighbour k
D2 = (0, 0, -1, -1, -1, 0, 1, 1, 1)    # dy of neighbour k


def _nb(a, k, fill):
    dy, dx = D2[k], D1[k]
    out = np.full_like(a, fill)
    H, W = a.shape
    y0, y1 = max(0, -dy), H - max(0, dy)
    x0, x1 = max(0, -dx), W - max(0, dx)
    out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def classify(z, nodata=NODATA):
    """queue (D8 first pass: an interior cell without a nodata neighbour and without a lower neighbour), incfall / incrise seeds and masks
    (flatk::classify_stream_kernel; dontCross is not modelled - it cannot fire inside a lake, where no cell has a direction)"""
    ny, nx = z.shape
    valid = z != nodata
    interior = np.zeros_like(valid)
    interior[1:-1, 1:-1] = True
    ok = interior & valid
    lower = np.zeros_like(valid)
    for k in range(1, 9):
        ok &= _nb(valid, k, False)
        lower |= _nb(z, k, np.float32(np.inf)) < z
    q = ok & ~lower
    hasdir = ok & lower
    low = np.zeros_like(q); quirk = np.zeros_like(q); higher = np.zeros_like(q)
    fm = np.zeros(z.shape, np.uint8); rm = np.zeros(z.shape, np.uint8)
    for k in range(1, 9):
        zn, qn, hn = _nb(z, k, np.float32(-np.inf)), _nb(q, k, False), _nb(hasdir, k, False)
        zd = z - zn
        low |= q & (zd >= 0) & hn
        eq = q & (zd == 0) & ~hn
        fm |= (eq & qn).astype(np.uint8) << (k - 1)
        quirk |= eq & ~qn
        higher |= q & (zd < 0)
        rm |= (q & qn).astype(np.uint8) << (k - 1)
    fm[low] = 0
    rm[higher] = 0
    lvl = np.where(q, np.where(low, 1, np.where(quirk, 2, 0)), -1).astype(np.int32)
    rq = np.where(q, np.where(higher, 1, 0), -1).astype(np.int32)
    return dict(q=q, lvl=lvl, rq=rq, fm=fm, rm=rm)


def full_tiles(mask, y_lo=None, y_hi=None):
    """per complete tile (a partial last tile row / column never is one): every cell's mask is 0xFF; rows outside [y_lo, y_hi) (a strip's boundary tile
    rows) excluded as flats_bfs does"""
    ny, nx = mask.shape
    ty, tx = ny // TS, nx // TS
    y_lo = 0 if y_lo is None else y_lo
    y_hi = ny if y_hi is None else y_hi
    f = (mask[:ty * TS, :tx * TS] == 0xFF).reshape(ty, TS, tx, TS).all(axis=(1, 3))
    out = np.zeros(((ny + TS - 1) // TS, (nx + TS - 1) // TS), bool)
    out[:ty, :tx] = f
    rows = np.arange(out.shape[0])
    out[(rows * TS < y_lo) | ((rows + 1) * TS > y_hi)] = False
    return out


def find_blocks(full, kmax=8):
    """flatk::find_blocks_kernel: per aligned 8 x 8 region the largest aligned blocks of full tiles (8, then 4, then 2).  Returns {(tx, ty): K} of the
    blocks' first tiles and the map tile -> first tile of its block."""
    tiles_y, tiles_x = full.shape
    blocks, owner = {}, {}
    for by0 in range(0, tiles_y, 8):
        for bx0 in range(0, tiles_x, 8):
            for j in range(8):
                for i in range(8):
                    tx, ty = bx0 + i, by0 + j
                    if tx >= tiles_x or ty >= tiles_y:
                        continue
                    kk = kmax
                    while kk >= 2:
                        i0, j0 = i & ~(kk - 1), j & ~(kk - 1)
                        x0, y0 = bx0 + i0, by0 + j0
                        if x0 + kk <= tiles_x and y0 + kk <= tiles_y and full[y0:y0 + kk, x0:x0 + kk].all():
                            owner[(tx, ty)] = (x0, y0)
                            if (i, j) == (i0, j0):
                                blocks[(tx, ty)] = kk
                            break
                        kk >>= 1
    return blocks, owner


def first_round_entries(q, blocks, owner):
    """the list of round 0: every tile with a queue cell, a block's tiles once (block_flags_kernel)"""
    ny, nx = q.shape
    tq = np.zeros(((ny + TS - 1) // TS, (nx + TS - 1) // TS), bool)
    yy, xx = np.nonzero(q)
    tq[yy // TS, xx // TS] = True
    ents = set()
    for ty, tx in zip(*np.nonzero(tq)):
        ents.add(owner.get((int(tx), int(ty)), (int(tx), int(ty))))
    return len(ents)


# ---- the sweep: every (K, E, j, source) of the closed form's branch edges ----
def positions(k):
    W = 64 * k
    return sorted({0, 1, 2, 63, 64, 65, 127, 128, 129, W - 1, W, W + 1})


def sweep_lakes(k, source, regions_x):
    """one lake per (E, j) in its own 8 x 8-tile region, laid out row by row; K = 8 blocks fill a region, so their lakes sit in every other region"""
    lakes = []
    step = 2 if k == 8 else 1
    off = {2: 2, 4: 4, 8: 0}[k]        # K < 8: the block 2 / 4 tiles into its region
    n = 0
    for E in range(4):
        for j in positions(k):
            rx, ry = (n % regions_x) * step + (1 if k == 8 else 0), (n // regions_x) * step + (1 if k == 8 else 0)
            n += 1
            kw = dict(fall=((E, j),)) if source == "fall" else dict(rise=((E, j),), margin=2)
            lakes.append(Lake(k, rx * 8 + off, ry * 8 + off, **kw))
    return lakes


def sweep_raster(k, source):
    regions_x = 6 if k == 8 else 8
    lakes = sweep_lakes(k, source, regions_x)
    nreg_y = (len(lakes) + regions_x - 1) // regions_x
    if k == 8:
        shape = ((2 * nreg_y + 1) * 512 + 37, (2 * regions_x + 1) * 512 + 37)
    else:
        shape = (nreg_y * 512 + 37, regions_x * 512 + 37)
    return make_dem(shape, lakes, rough=ROUGH), lakes


def race_raster():
    lakes = race_lakes([(i % 4, i // 4) for i in range(6)])
    return make_dem((2 * 512 + 37, 4 * 512 + 37), lakes, rough=ROUGH), lakes


def race_lakes(regions):
    """One-sided activations: ring edge 0's only level-1 seeds lie at positions >= 64 (waves 1 - 3 of the block update, none in wave 0), and a seed on
    edge 2 holds the rim low near edge 0's positions 0 .. 63 - if edge 0's flag were lost in an activation, the ring cells there would never wake the
    block again (the moved[] zero / flag race)."""
    specs = [(2, ((0, 128), (2, 32))), (2, ((0, 65), (2, 40))), (4, ((0, 192), (2, 32))), (4, ((0, 128), (3, 20))), (2, ((1, 100), (3, 30))),
             (4, ((3, 200), (0, 10)))]
    out = []
    for n, (k, fall) in enumerate(specs[:len(regions)]):
        rx, ry = regions[n]
        out.append(Lake(k, rx * 8 + k, ry * 8 + k, fall=fall))
    return out


SHAPES = {   # (ny, nx): tiles_x % 8 == 0 or not, nx = 64 m - 1, 64 m, 64 m + 1 / + 2, partial last tile rows of 1, 2 and 63 rows
    "vec_64m": (64 * 8 + 2, 64 * 16),          # tiles_x 16: find_blocks_kernel's 16-byte path; a block in the last complete tile row (its wall is the border row)
    "scalar_64m+2": (64 * 9 + 1, 64 * 16 + 2),  # tiles_x 17: the scalar path; a block in the last complete tile column (its wall is the border column)
    "vec_64m-1": (64 * 10 - 1, 64 * 16 - 1),     # tiles_x 16, a partial last tile column and row of 63 cells that a lake reaches into
    "scalar_64m+1": (64 * 17 + 1, 64 * 24 + 1),  # tiles_x 25, a partial last tile row of one row
}


def shapes_lakes(name):
    """blocks in the first and last complete tile row / column a block can take (a block's ring and wall are the two cells outside it), two blocks chained
    through each other's ring, islands that cut an 8 x 8 block down to 4 and 2, an undrained lake, a nodata shore, a lake reaching into a partial tile"""
    ny, nx = SHAPES[name]
    tiles_x, tiles_y = nx // TS, ny // TS               # complete tiles
    lakes = [Lake(2, 2, 2, fall=((2, 1),))]                # the first tile row and column a block can start in (tiles 0 and 1 hold the border and the ring)
    if name == "vec_64m":
        lakes += [Lake(2, 6, tiles_y - 2, fall=((0, 64),)),           # last complete tile row: ring row 512, wall = border row 513
                  Lake(2, 6, 2, nbx=2, fall=((2, 64),)),              # two blocks side by side: each one's ring is the other's rim
                  Lake(2, 12, 4, fall=()),                            # undrained: incfall never reaches the lake
                  ]
    elif name == "scalar_64m+2":
        lakes += [Lake(2, tiles_x - 2, 4, fall=((1, 3),)),            # last complete tile column: ring column 1024, wall = border column 1025
                  Lake(4, 8, 4, margin=2, nodata=True, rise=((2, 100),)),
                  ]
    elif name == "vec_64m-1":
        # flats that run into the partial tile column 15 / row 9 (63 cells): tiles 14 - 15 and rows 8 - 9 can never be a block
        lakes += [Lake(2, 14, 2, fall=((2, 5),), blocks=(), clip=True),
                  Lake(2, 4, 8, fall=((0, 5),), blocks=(), clip=True),
                  Lake(4, 8, 4, fall=((3, 70),))]                    # (deeper than the clipped lakes: its blocks shorten the rounds)
    elif name == "scalar_64m+1":
        # an 8 x 8 region with an island in tile (7, 7): blocks of 4, 4, 4 and 2, 2, 2 in one region
        lakes += [Lake(8, 8, 8, fall=((1, 100),), islands=((7 * 64 + 20, 7 * 64 + 20, 5, 7),),
                       blocks=((8, 8, 4), (12, 8, 4), (8, 12, 4), (12, 12, 2), (14, 12, 2), (12, 14, 2)))]
    return lakes


def shapes_raster(name):
    lakes = shapes_lakes(name)
    return make_dem(SHAPES[name], lakes, rough=ROUGH), lakes


def lake_window(lake, shape):
    """a window of the raster around a lake that starts on an 8 x 8-tile region's corner (so the model's regions are the raster's)"""
    wy0, wy1, wx0, wx1 = lake.box(lake.margin + 2)
    y0, x0 = max(0, (wy0 - 1) // 512 * 512), max(0, (wx0 - 1) // 512 * 512)
    y1, x1 = min(shape[0], -(-(wy1 + 1) // TS) * TS), min(shape[1], -(-(wx1 + 1) // TS) * TS)
    if lake.clip:
        y1, x1 = shape
    return y0, y1, x0, x1


def lake_model(z, lake, kmax=8, whole=False):
    """what the model says of one lake: its blocks per field ({(tx, ty): K}, raster tile coordinates) and the ring cells holding level 1 per field
    and edge"""
    y0, y1, x0, x1 = (0, z.shape[0], 0, z.shape[1]) if whole else lake_window(lake, z.shape)
    w = z[y0:y1, x0:x1]
    c = classify(w)   # (the window's own border is ground far from the lake: what the model makes of it there does not matter)
    out = {}
    wy0, wy1, wx0, wx1 = lake.box(lake.margin + 2)
    for field, mask, lev in (("fall", c["fm"], c["lvl"]), ("rise", c["rm"], c["rq"])):
        blocks, _ = find_blocks(full_tiles(mask), kmax)
        mine = {(tx + x0 // TS, ty + y0 // TS): k for (tx, ty), k in blocks.items()
                if wy0 <= (ty + y0 // TS) * TS < wy1 and wx0 <= (tx + x0 // TS) * TS < wx1}
        ring1 = {E: [j for j, (y, x) in enumerate(lake.ring_cells(E)) if 0 <= y - y0 < w.shape[0] and 0 <= x - x0 < w.shape[1] and lev[y - y0, x - x0] == 1]
                 for E in range(4)}
        fy0, fy1, fx0, fx1 = lake.box(lake.margin + 1)
        inner = lev[max(fy0 - y0, 0):fy1 - y0, max(fx0 - x0, 0):fx1 - x0]
        out[field] = dict(blocks=mine, ring1=ring1, seeds=int((inner > 0).sum()), queued=int((inner >= 0).sum()))
    return out
