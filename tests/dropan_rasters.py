"""Hand-written p / fel / ssa rasters for the DropAnalysis tests: junctions with chosen inflow orders in neighbour order, junctions on tile corners, and the
mask's edge cases.  Cells of the network have ssa = 10 (a few 0 or nodata where a case wants it) and every other cell ssa = 0 and no direction, so that
any threshold in (0, 10] cuts exactly the network."""
import numpy as np

P_NODATA = -32768
SSA_NODATA = -1.0
DX = (0, 1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, 0, -1, -1, -1, 0, 1, 1, 1)
CODE = {(DX[k], DY[k]): k for k in range(1, 9)}


class _Net:
    def __init__(self, shape, seed):
        self.p = np.full(shape, P_NODATA, np.int16)
        self.ssa = np.zeros(shape, np.float32)
        rng = np.random.default_rng(seed)
        self.fel = (rng.random(shape) * 100.0 + 50.0).astype(np.float32)

    def cell(self, x, y, to, ssa=10.0):
        """cell (x, y) on the network, draining to the neighbouring cell `to` (None: no direction)"""
        assert self.p[y, x] == P_NODATA and self.ssa[y, x] == 0.0, f"cell ({x}, {y}) used twice"
        if to is not None:
            self.p[y, x] = CODE[to[0] - x, to[1] - y]
        else:
            self.p[y, x] = 0
        self.ssa[y, x] = ssa

    def arm(self, x, y, k, order):
        """a stream of `order` (1 or 2) that enters (x, y) from neighbour k: two cells, and for order 2 two sources beside the outer one"""
        a1, a2 = (x + DX[k], y + DY[k]), (x + 2 * DX[k], y + 2 * DY[k])
        self.cell(*a1, (x, y))
        self.cell(*a2, a1)
        if order == 2:
            px, py = (-DY[k], DX[k])                # perpendicular
            self.cell(a2[0] + px, a2[1] + py, a2)
            self.cell(a2[0] - px, a2[1] - py, a2)
        else:
            assert order == 1

    def rasters(self):
        return self.p, self.fel, self.ssa


def junction(orders, ks=(1, 3, 5, 7), at=(10, 10), shape=(21, 21), seed=5):
    """p, fel, ssa, (x, y): a junction at `at` whose inflows come from the neighbours `ks` (ascending: the scan order) with the given orders; it drains through
    a short stream to the south-east"""
    assert list(ks) == sorted(ks) and len(ks) == len(orders) and 8 not in ks
    n = _Net(shape, seed)
    x, y = at
    for k, o in zip(ks, orders):
        n.arm(x, y, k, o)
    n.cell(x, y, (x + 1, y + 1))
    n.cell(x + 1, y + 1, (x + 2, y + 2))
    n.cell(x + 2, y + 2, None)
    return n.rasters() + (at,)


def two_junctions():
    """(1,1,2,2) at (10, 10) and (2,2,1,1) at (30, 10) in one raster"""
    a = junction((1, 1, 2, 2), shape=(21, 41))
    b = junction((2, 2, 1, 1), at=(30, 10), shape=(21, 41), seed=6)
    p = np.where(b[0] != P_NODATA, b[0], a[0])
    return p, a[1], np.maximum(a[2], b[2]), ((10, 10), (30, 10))


def tile_corners():
    """junctions whose inflows sit on both sides of the 64-cell tile corner (64, 64) and of the 32-cell corner (32, 32): 80 x 80"""
    a = junction((1, 2, 1), ks=(3, 4, 5), at=(64, 64), shape=(80, 80), seed=7)
    b = junction((2, 2, 1), ks=(3, 4, 5), at=(32, 32), shape=(80, 80), seed=7)
    p = np.where(b[0] != P_NODATA, b[0], a[0])
    return p, a[1], np.maximum(a[2], b[2]), ((64, 64), (32, 32))


def _row_stream(ssa_of_third, cycle=False):
    """two streams that flow east along rows 3 and 6 of a 12 x 40 raster and meet at (30, 5); cell (10, 3) of the first one takes `ssa_of_third`"""
    n = _Net((12, 40), 9)
    for x in range(2, 29):
        n.cell(x, 3, (x + 1, 3), ssa_of_third if x == 10 else 10.0)
        n.cell(x, 6, (x + 1, 6))
    n.cell(29, 3, (30, 4))
    n.cell(30, 4, (30, 5))
    n.cell(29, 6, (30, 5))
    n.cell(30, 5, (31, 5))
    for x in range(31, 37):
        n.cell(x, 5, (x + 1, 5) if x < 36 else None)
    for x in (5, 15, 20):                  # side branches: more junctions, first-order and higher-order drops
        n.cell(x, 1, (x, 2))
        n.cell(x, 2, (x, 3))
        n.cell(x + 1, 8, (x + 1, 7))
        n.cell(x + 1, 7, (x + 1, 6))
    if cycle:                              # two cells that point at each other, fed by a source and feeding nobody: never evaluated
        n.cell(20, 10, (21, 10))
        n.cell(21, 10, (20, 10))
        n.cell(19, 10, (20, 10))
    return n.rasters()


def off_mask_gap():
    """a mask cell drains into an off-mask cell (ssa 0) and the stream comes back onto the mask: the cell after the gap is a source"""
    return _row_stream(0.0)


def ssa_nodata_gap():
    """the same with ssa nodata inside the stream"""
    return _row_stream(SSA_NODATA)


def with_cycle():
    return _row_stream(10.0, cycle=True)
