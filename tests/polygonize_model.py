"""The definition of the watershed polygons (include/taudem_amd_polygonize.h) in plain numpy / Python, and its own checkers.

The model finds successors GEOMETRICALLY: among the boundary edges of the same id that start at the vertex where an edge ends it prefers the one that
turns right, then the one straight on, then the one that turns left.  It does not use the cell-local rule of the device code.  It assigns a hole to its
polygon through a flood fill of the 4-connected pieces, not through the walk up a column of the host code.

polygonize(w) -> Model: the edge columns (keys ascending, successor keys, ids) and the layer as offset lists, the arrays Context.polygonize returns.
check(w, model): the rings fill back to exactly w == id (cumulative sum of the signed vertical edges per row), cells is the count of w == id, and every
id has as many polygons as 4-connected pieces."""
from collections import namedtuple

import numpy as np

NODATA = -2147483647
# side 0 top (east), 1 right (south), 2 bottom (west), 3 left (north): start vertex offset and step (dc, dr)
START = ((0, 0), (1, 0), (1, 1), (0, 1))
STEP = ((1, 0), (0, 1), (-1, 0), (0, -1))

Model = namedtuple("Model", "keys next_keys edge_ids ids cells poly_first ring_first vert_first vertices")


def boundary_edges(w, nodata=NODATA):
    """[(key, id, start vertex, end vertex, direction)] ascending by key."""
    w = np.asarray(w)
    ny, nx = w.shape
    pad = np.full((ny + 2, nx + 2), nodata, dtype=np.int64)
    valid = np.zeros((ny + 2, nx + 2), dtype=bool)
    pad[1:-1, 1:-1] = w
    valid[1:-1, 1:-1] = w != nodata
    me, ok = pad[1:-1, 1:-1], valid[1:-1, 1:-1]
    out = []
    # neighbour across side s: N, E, S, W
    for s, (dr, dc) in enumerate(((-1, 0), (0, 1), (1, 0), (0, -1))):
        nb = pad[1 + dr:ny + 1 + dr, 1 + dc:nx + 1 + dc]
        nbok = valid[1 + dr:ny + 1 + dr, 1 + dc:nx + 1 + dc]
        rr, cc = np.nonzero(ok & (~nbok | (nb != me)))
        for r, c in zip(rr.tolist(), cc.tolist()):
            v0 = (c + START[s][0], r + START[s][1])
            out.append(((r * nx + c) * 4 + s, int(w[r, c]), v0, (v0[0] + STEP[s][0], v0[1] + STEP[s][1]), s))
    out.sort()
    return out


def pieces(w, nodata=NODATA):
    """label grid of the 4-connected pieces of equal id (-1 on nodata) and {id: number of pieces}, by flood fill."""
    w = np.asarray(w)
    ny, nx = w.shape
    lab = np.full((ny, nx), -1, dtype=np.int64)
    count = {}
    n = 0
    wl = w.tolist()
    for r0 in range(ny):
        for c0 in range(nx):
            a = wl[r0][c0]
            if a == nodata or lab[r0, c0] >= 0:
                continue
            count[a] = count.get(a, 0) + 1
            lab[r0, c0] = n
            stack = [(r0, c0)]
            while stack:
                r, c = stack.pop()
                for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                    if 0 <= rr < ny and 0 <= cc < nx and lab[rr, cc] < 0 and wl[rr][cc] == a:
                        lab[rr, cc] = n
                        stack.append((rr, cc))
            n += 1
    return lab, count


def shoelace2(ring):
    """twice the signed area of a closed ring of (c, r): positive for an outer ring (clockwise in map view, where y runs against r)."""
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring[:-1], ring[1:]))


def rings_of(edges):
    """[(id, ring)] with ring = [(c, r), ...]: corners only, from the smallest vertex by (r, c), closed.  Also asserts that the geometric successor map
    is a permutation."""
    starts = {}
    for i, (_, a, v0, _, d) in enumerate(edges):
        starts.setdefault((v0, a), {})[d] = i
    succ = []
    for _, a, _, v1, d in edges:
        cand = starts[(v1, a)]
        succ.append(next(cand[t] for t in ((d + 1) % 4, d, (d + 3) % 4) if t in cand))
    assert sorted(succ) == list(range(len(edges))), "the successor map is not a permutation"
    seen = [False] * len(edges)
    out = []
    for i0 in range(len(edges)):
        if seen[i0]:
            continue
        cyc, i = [], i0
        while not seen[i]:
            seen[i] = True
            cyc.append(i)
            i = succ[i]
        assert i == i0
        corners = [edges[i][2] for k, i in enumerate(cyc) if edges[i][4] != edges[cyc[k - 1]][4]]
        s = min(range(len(corners)), key=lambda k: (corners[k][1], corners[k][0]))
        ring = corners[s:] + corners[:s]
        out.append((edges[i0][1], ring + ring[:1]))
    return succ, out


def polygonize(w, nodata=NODATA):
    w = np.asarray(w)
    edges = boundary_edges(w, nodata)
    succ, rings = rings_of(edges)
    lab, _ = pieces(w, nodata)
    outer, holes = {}, {}   # piece label -> ring / rings
    for a, ring in rings:
        c0, r0 = ring[0]
        if shoelace2(ring) > 0:
            assert w[r0, c0] == a and lab[r0, c0] not in outer
            outer[int(lab[r0, c0])] = (a, ring)
        else:
            assert w[r0 - 1, c0] == a
            holes.setdefault(int(lab[r0 - 1, c0]), []).append(ring)
    start = lambda ring: (ring[0][1], ring[0][0])  # noqa: E731
    ids, cells, poly_first, ring_first, vert_first, verts = [], [], [0], [0], [0], []
    for a, _, ring, piece in sorted((a, start(ring), ring, piece) for piece, (a, ring) in outer.items()):
        if not ids or ids[-1] != a:
            if ids:
                poly_first.append(len(ring_first) - 1)
            ids.append(a)
            cells.append(0)
        group = [ring] + sorted(holes.get(piece, []), key=start)
        for g in group:
            cells[-1] += shoelace2(g)
            verts += g
            vert_first.append(len(verts))
        ring_first.append(len(vert_first) - 1)
    if ids:
        poly_first.append(len(ring_first) - 1)
    assert set(holes) <= set(outer)
    return Model(np.array([e[0] for e in edges], np.int64), np.array([edges[i][0] for i in succ], np.int64), np.array([e[1] for e in edges], np.int32),
                 np.array(ids, np.int32), np.array([c // 2 for c in cells], np.int64), np.array(poly_first, np.int64), np.array(ring_first, np.int64),
                 np.array(vert_first, np.int64), np.array(verts, np.int32).reshape(-1, 2))


def features(m):
    """[(id, cells, [polygon, ...])], polygon = [ring, ...], ring = [(c, r), ...]: the nesting of the offset lists."""
    out = []
    for f in range(len(m.ids)):
        polys = []
        for p in range(m.poly_first[f], m.poly_first[f + 1]):
            polys.append([[tuple(int(v) for v in xy) for xy in m.vertices[m.vert_first[q]:m.vert_first[q + 1]]] for q in range(m.ring_first[p], m.ring_first[p + 1])])
        out.append((int(m.ids[f]), int(m.cells[f]), polys))
    return out


def fill_back(rings, ny, nx):
    """The cells inside a set of rings: +1 at a vertical edge that runs north (the id lies east of it), -1 at one that runs south, summed along the row."""
    d = np.zeros((ny, nx + 1), dtype=np.int64)
    for ring in rings:
        for (c0, r0), (c1, r1) in zip(ring[:-1], ring[1:]):
            assert (c0 == c1) != (r0 == r1), "a ring edge is axis-parallel and not empty"
            if c0 == c1:
                if r1 < r0:
                    d[r1:r0, c0] += 1
                else:
                    d[r0:r1, c0] -= 1
    inside = np.cumsum(d, axis=1)
    assert not inside[:, nx].any()
    return inside[:, :nx]


def check(w, m, nodata=NODATA):
    """The model's (or the library's) layer against the grid."""
    w = np.asarray(w)
    ny, nx = w.shape
    _, count = pieces(w, nodata)
    feats = features(m)
    assert [f[0] for f in feats] == sorted(count), "one feature per id, ascending"
    for a, cells, polys in feats:
        assert len(polys) == count[a], f"id {a}: {len(polys)} polygons, {count[a]} pieces"
        assert [p[0][0][::-1] for p in polys] == sorted(p[0][0][::-1] for p in polys), "polygons by start vertex"
        for p in polys:
            assert shoelace2(p[0]) > 0 and all(shoelace2(h) < 0 for h in p[1:])
            assert [h[0][::-1] for h in p[1:]] == sorted(h[0][::-1] for h in p[1:]), "holes by start vertex"
            for ring in p:
                assert ring[0] == ring[-1] and ring[0] == min(ring, key=lambda v: (v[1], v[0])) and len(ring) >= 5
            inside = fill_back(p, ny, nx)
            assert set(np.unique(inside)) <= {0, 1}
        inside = fill_back([r for p in polys for r in p], ny, nx)
        assert np.array_equal(inside == 1, w == a), f"id {a}: the rings do not fill back to w == id"
        assert cells == int((w == a).sum())
    assert m.poly_first[0] == 0 and m.ring_first[0] == 0 and m.vert_first[0] == 0
    assert m.poly_first[-1] == len(m.ring_first) - 1 and m.ring_first[-1] == len(m.vert_first) - 1 and m.vert_first[-1] == len(m.vertices)


def same(a, b):
    """Two layers (Model, or anything with the same array attributes) hold exactly the same arrays."""
    for name in ("ids", "cells", "poly_first", "ring_first", "vert_first", "vertices"):
        x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
        assert x.shape == y.shape and np.array_equal(x, y), name
    return True


# ---- the hand cases
def hand_cases():
    nd = NODATA
    nested = np.full((9, 10), 1, np.int32)
    nested[2:7, 2:8] = 2
    nested[4, 4:6] = 1
    nested[0, 0] = nd
    stripes = np.fromfunction(lambda r, c: (r + c) % 3, (7, 9), dtype=np.int64).astype(np.int32)
    checker = np.fromfunction(lambda r, c: 1 + (r + c) % 2, (6, 5), dtype=np.int64).astype(np.int32)
    cut = np.array([[1, 1, 1, 1, 1, 2],     # regions, a saddle and a hole on rows 2 and 3, where a cut at 3 (or per row) falls
                    [1, 3, 3, 3, 1, 2],
                    [1, 3, nd, 3, 1, 1],
                    [1, 3, 3, 3, 2, 1],
                    [1, 1, 1, 2, 1, 1],
                    [-5, 0, 0, 1, 1, -5]], np.int32)
    return {
        "one_cell": np.array([[7]], np.int32),
        "saddle": np.array([[1, 2], [2, 1]], np.int32),
        "ring_around_nodata": np.array([[1, 1, 1], [1, nd, 1], [1, 1, 1]], np.int32),
        "nested": nested,
        "stripes": stripes,
        "checker": checker,
        "all_nodata": np.full((3, 4), nd, np.int32),
        "single_id": np.full((4, 3), -3, np.int32),
        "negative_and_zero": np.array([[0, 0, -1], [-1, 0, -1], [-2147483648, 2147483647, 0]], np.int32),
        "cut": cut,
    }
