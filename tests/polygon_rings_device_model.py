"""The schedule of the device ring builder (taudem_amd/csrc/polygon_rings_device.hip) restated in numpy, array operation for kernel: what can be held
to the definition (tests/polygonize_model.py) on a machine without a GPU.

build(keys, next_keys, ids, nx, ny) -> (Model-like layer, Rounds).  The steps and their names are the kernels':
  successor   next key -> edge index by binary search; the refusals; the corner mark scattered through the permutation (one writer per slot)
  label       min-jump rounds on the cyclic permutation with the state (m, j, off, w): m the smallest edge index within 2^k steps, j the 2^k-th
              successor, w the corners within 2^k steps, off the corners before the first place m was seen.  A round that changes no m ends them.
  per ring    corners, smallest vertex, signed area (x dy over the vertical edges)
  rank        rotation = rank of the smallest vertex; position = (rank - rotation) mod corners
  holes       up the column of the start vertex to the first top edge; parent = that edge's ring; parents jumped to the outer ring
  order       stable sorts by own start, owner's start, id (numpy's lexsort); scans

round_bound(E) is the bound the kernels use: ceil(log2(E)) + 1.  The device reads its "changed" word every second round, so it runs
device_rounds(needed, bound) rounds, which is still within the bound."""
from collections import namedtuple

import numpy as np

Layer = namedtuple("Layer", "ids cells poly_first ring_first vert_first vertices")
Rounds = namedtuple("Rounds", "label bound owner owner_bound")


class Refused(ValueError):
    pass


def round_bound(n):
    """ceil(log2(n)) + 1 for n >= 1."""
    b = 1
    while (1 << (b - 1)) < n:
        b += 1
    return b


def device_rounds(needed, bound):
    """The rounds the device runs when `needed` rounds end with one that changes nothing: it looks after every second round and after the last."""
    return min(bound, needed + (needed & 1))


def _empty():
    z = np.zeros(1, np.int64)
    return Layer(np.zeros(0, np.int32), np.zeros(0, np.int64), z, z.copy(), z.copy(), np.zeros((0, 2), np.int32))


def build(keys, next_keys, ids, nx, ny):
    keys, next_keys, ids = np.asarray(keys, np.int64), np.asarray(next_keys, np.int64), np.asarray(ids, np.int32)
    E = len(keys)
    if E == 0:
        return _empty(), Rounds(0, 0, 0, 0)
    # ---- successor, validate
    if ((keys < 0) | (keys >= 4 * nx * ny)).any():
        raise Refused("an edge key outside the raster")
    if (keys[1:] <= keys[:-1]).any():
        raise Refused("edge keys do not ascend")
    at = np.searchsorted(keys, next_keys)
    found = (at < E) & (keys[np.minimum(at, E - 1)] == next_keys)
    if not found.all():
        raise Refused("the successor of an edge is not among the edges")
    nxt = at
    side, cell = keys & 3, keys >> 2
    r, c = cell // nx, cell % nx
    vc, vr = c + ((side == 1) | (side == 2)), r + ((side == 2) | (side == 3))           # start vertex
    ec, er = c + ((side == 0) | (side == 1)), r + ((side == 1) | (side == 2))           # end vertex: the start of side + 1
    if ((ec != vc[nxt]) | (er != vr[nxt])).any():
        raise Refused("a successor does not start where its edge ends")
    if (ids[nxt] != ids).any():
        raise Refused("the id changes along a ring")
    mark = np.zeros(E, np.uint8)
    mark[nxt] = 1 + (side[nxt] != side)
    if (mark == 0).any():
        raise Refused("the successors are not a permutation of the edges")
    corner = mark == 2
    # ---- label
    m, j, off, w = np.arange(E, dtype=np.int64), nxt.astype(np.int64), np.zeros(E, np.int64), corner.astype(np.int64)
    bound, needed = round_bound(E), None
    for k in range(bound):
        tm, tj, toff, tw = m[j], j[j], off[j], w[j]
        ch = tm < m
        off = np.where(ch, w + toff, off)
        m = np.where(ch, tm, m)
        w = w + tw
        j = tj
        if not ch.any():
            needed = k + 1
            break
    if needed is None:   # the windows cover 2^bound >= 2 E edges: every cycle twice
        needed = bound
    lead = m == np.arange(E)
    rid = np.cumsum(lead) - lead
    ring_of = rid[m]
    R = int(lead.sum())
    # ---- per ring
    nv = np.bincount(ring_of, weights=corner, minlength=R).astype(np.int64)
    packed = (vr << 32) | vc
    vmin = np.full(R, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(vmin, ring_of[corner], packed[corner])
    area = np.zeros(R, np.int64)
    np.add.at(area, ring_of, np.where(side == 1, vc, np.where(side == 3, -vc, 0)))
    ring_id = ids[lead]
    if (nv < 4).any():
        raise Refused("a ring of fewer than four corners")
    if (area == 0).any():
        raise Refused("a ring without area")
    # ---- rank
    rank = (nv[ring_of] - off % nv[ring_of]) % nv[ring_of]
    first = corner & (packed == vmin[ring_of])
    assert np.array_equal(np.sort(ring_of[first]), np.arange(R)), "a ring passes its smallest vertex once"
    rot = np.zeros(R, np.int64)
    rot[ring_of[first]] = rank[first]
    # ---- holes
    r0, c0 = vmin >> 32, vmin & 0xffffffff
    parent = np.arange(R)
    holes = np.nonzero(area < 0)[0]
    for h in holes.tolist():
        p = -1
        if c0[h] < nx:
            rows = np.arange(r0[h] - 1, -1, -1)
            k = (rows * nx + c0[h]) * 4
            e = np.searchsorted(keys, k)
            hit = (e < E) & (keys[np.minimum(e, E - 1)] == k)
            if hit.any():
                q = ring_of[e[np.argmax(hit)]]
                if ring_id[q] == ring_id[h]:
                    p = q
        if p < 0:
            raise Refused("a hole without an outer ring")
        parent[h] = p
    owner_bound, owner_needed = round_bound(len(holes) + 1), 0
    if len(holes):
        owner_needed = None
        for k in range(owner_bound):
            pp = parent[parent]
            same = np.array_equal(pp, parent)
            parent = pp
            if same:
                owner_needed = k + 1
                break
        if owner_needed is None:
            owner_needed = owner_bound
        assert (area[parent] > 0).all(), "every owner is an outer ring"
    # ---- order
    vkey = lambda q: r0[q] * (nx + 1) + c0[q]  # noqa: E731
    order = np.lexsort((vkey(np.arange(R)), vkey(parent), ring_id.astype(np.int64)))
    inv = np.empty(R, np.int64)
    inv[order] = np.arange(R)
    nvc = nv[order] + 1
    vert_first = np.concatenate([[0], np.cumsum(nvc)]).astype(np.int64)
    outer = area[order] > 0
    sid = ring_id[order]
    feat = outer & np.concatenate([[True], sid[1:] != sid[:-1]])
    assert outer[0] and feat[0], "the order starts with an outer ring"
    pidx, fidx = np.cumsum(outer) - outer, np.cumsum(feat) - feat
    P, F = int(outer.sum()), int(feat.sum())
    ring_first = np.concatenate([np.nonzero(outer)[0], [R]]).astype(np.int64)
    poly_first = np.concatenate([pidx[feat], [P]]).astype(np.int64)
    out_ids = sid[feat].astype(np.int32)
    cells = np.zeros(F, np.int64)
    np.add.at(cells, fidx + feat - 1, area[order])
    # ---- scatter
    vert = np.full((int(vert_first[-1]), 2), -1, np.int32)
    q = ring_of[corner]
    pos = (rank[corner] + nv[q] - rot[q]) % nv[q]
    slot = vert_first[inv[q]] + pos
    assert len(np.unique(slot)) == len(slot), "one writer per slot"
    vert[slot, 0], vert[slot, 1] = vc[corner], vr[corner]
    z = pos == 0
    vert[slot[z] + nv[q][z], 0], vert[slot[z] + nv[q][z], 1] = vc[corner][z], vr[corner][z]
    assert (vert >= 0).all(), "every slot has a writer"
    return Layer(out_ids, cells, poly_first, ring_first, vert_first, vert), Rounds(needed, bound, owner_needed, owner_bound)
