"""The contract of include/taudem_amd_regions.h in numpy: the SINMAP parameter region grid.  Every crossing is evaluated for every cell of the rows a
feature can reach, with the header's double operations in the header's order (numpy rounds after every ufunc: nothing is contracted).  No bitmaps, no
scans, no batches: nothing of the product's method."""
import numpy as np


def ring_edges(ring, gt):
    """px1, py1, px2, py2 of a ring's edges in pixel coordinates; None for a ring of fewer than 3 distinct vertices.  An open ring is closed."""
    r = np.asarray(ring, np.float64).reshape(-1, 2)
    if len({(float(a), float(b)) for a, b in r}) < 3:
        return None
    if r[0, 0] != r[-1, 0] or r[0, 1] != r[-1, 1]:
        r = np.vstack([r, r[:1]])
    px = (r[:, 0] - gt[0]) / gt[1]
    py = (r[:, 1] - gt[3]) / gt[5]
    if not (np.isfinite(px).all() and np.isfinite(py).all()):
        raise ValueError("a vertex without finite pixel coordinates")
    return px[:-1], py[:-1], px[1:], py[1:]


def inside(shape, gt, rings, row0=0):
    """bool (ny, nx): the cells of rows row0 .. row0 + ny - 1 whose centres the feature holds, by the even-odd rule over all its rings."""
    ny, nx = shape
    count = np.zeros((ny, nx), np.int64)
    xc = np.arange(nx, dtype=np.float64) + 0.5
    for ring in rings:
        e = ring_edges(ring, gt)
        if e is None:
            continue
        px1, py1, px2, py2 = (a[:, None] for a in e)
        lo, hi = np.minimum(py1, py2), np.maximum(py1, py2)
        if not lo.size:
            continue
        # rows outside this window have no crossing: their centres lie below every lo or not below any hi
        r0 = int(np.clip(np.floor(lo.min()) - 1 - row0, 0, ny))
        r1 = int(np.clip(np.ceil(hi.max()) + 1 - row0, 0, ny))
        if r1 <= r0:
            continue
        yc = (np.arange(row0 + r0, row0 + r1, dtype=np.float64) + 0.5)[None, :]
        crosses = (lo <= yc) & (yc < hi)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):   # an xs that overflows is -inf, +inf or NaN, and xs < xc holds as written
            xs = px1 + (yc - py1) * (px2 - px1) / (py2 - py1)
        left = crosses[:, :, None] & (xs[:, :, None] < xc[None, None, :])
        count[r0:r1] += left.sum(axis=0)
    return (count & 1) == 1


def ids_of(grid):
    return np.unique(grid[grid != 0]).astype(np.int32)


def polygons(shape, gt, features, values, row0=0):
    """grid (int16), ids: every cell the value of the LAST feature that holds its centre, 0 where none does."""
    if gt[2] != 0 or gt[4] != 0:
        raise ValueError("rotated geotransform")
    for k, v in enumerate(values):
        if not 1 <= int(v) <= 32767:
            raise ValueError(f"feature {k}: value {v} is outside 1 .. 32767")
    grid = np.zeros(shape, np.int16)
    for rings, v in zip(features, values):
        grid[inside(shape, gt, rings, row0)] = v
    return grid, ids_of(grid)


def resample(shape, gt, source, sgt, source_nodata):
    """grid, ids, bad: nearest neighbour; bad counts the cells that take a source value outside 1 .. 32767 (the call fails when it is not 0)."""
    ny, nx = shape
    sny, snx = source.shape
    c = np.arange(nx, dtype=np.float64)[None, :]
    r = np.arange(ny, dtype=np.float64)[:, None]
    x = gt[0] + (c + 0.5) * gt[1]
    y = gt[3] + (r + 0.5) * gt[5]
    sc = np.broadcast_to(np.floor((x - sgt[0]) / sgt[1]), shape)
    sr = np.broadcast_to(np.floor((y - sgt[3]) / sgt[5]), shape)
    on = (sc >= 0) & (sc < snx) & (sr >= 0) & (sr < sny)
    v = np.zeros(shape, np.int64)
    v[on] = source[sr[on].astype(np.int64), sc[on].astype(np.int64)]
    taken = on & (v != source_nodata)
    bad = int((taken & ((v < 1) | (v > 32767))).sum())
    grid = np.where(taken & (v >= 1) & (v <= 32767), v, 0).astype(np.int16)
    return grid, ids_of(grid), bad


def constant(shape):
    return np.ones(shape, np.int16), np.array([1], np.int32)


def table_text(ids, texts=("2.708", "2.708", "0.0", "0.25", "30.0", "45.0", "2000.0")):
    """The region table: the header line, then one line per id with the seven texts as given."""
    return "SiID,tmin,tmax,cmin,cmax,phimin,phimax,SoilDens\n" + "".join(f"{int(i)}," + ",".join(texts) + "\n" for i in ids)
