"""The device link builder of StreamNet (taudem_amd/csrc/streamnet_links_device.hip) restated in numpy, pass for kernel, and the host builder's FIFO walk
(taudem_amd/csrc/streamnet_links.cpp) restated literally beside it.  The device builder has no queue: the FIFO's pop order is the ascending order of

    h(c)     0 for a cell without a registered inflow (a seed), else 1 + the largest h of its inflows
    root(c)  the seed's own compact rank (the seeds enter the queue in that order), else the root of the inflow with the largest (h, root)

and everything else is local rules at the cells where links meet, pointer jumping along the cells with one inflow, a pass by levels over the link tree,
one sort and scans.  tests/test_streamnet_links_device_model.py holds build() to the reference's -tree / -coord bytes and to fifo() on random forests;
no GPU is needed.

    build(n, p, recv, flags, outlet)                        -> Model (label, order, the link table, the points, jump_rounds, level_rounds)
    rows(model, idx, nx, fel, ad8, length, dxA, dyA, gt)    -> tree int64 (links, 9), coord float64 (points, 5)
    fifo(n, p, recv, flags, outlet)                         -> (label, order, link table) of the host builder's walk
    read_compact(path)                                      -> the columns of a dump of the restatement (sn_dump_compact)
"""
from types import SimpleNamespace

import numpy as np

LINK_NONE = -2147483647
TERMINAL = 1


def read_compact(path):
    with open(path, "rb") as f:
        n = int(np.fromfile(f, np.int64, 1)[0])
        col = lambda t: np.fromfile(f, t, n)  # noqa: E731
        return SimpleNamespace(n=n, idx=col(np.int64), p=col(np.int16), fel=col(np.float32), ad8=col(np.float32), len=col(np.float32), outlet=col(np.int32),
                               recv=col(np.int32), flags=col(np.uint8))


def inflow_table(n, p, recv):
    """inflow[r, (k - 1 + 4) % 8] = u: a conflict-free scatter (one neighbour per direction)."""
    inflow = np.full((n, 8), -1, np.int64)
    u = np.arange(n)
    ok = (recv >= 0) & (recv != u) & (p >= 1) & (p <= 8)
    inflow[recv[ok], (p[ok].astype(np.int64) + 3) % 8] = u[ok]
    return inflow


def bubble(n_order, frm):
    """src/streamnet.cpp:839-851 exactly as written: two bubble passes."""
    k = len(n_order)
    for _ in range(2):
        for b in range(k - 1):
            if n_order[b] > n_order[b + 1]:
                n_order[b], n_order[b + 1] = n_order[b + 1], n_order[b]
                frm[b], frm[b + 1] = frm[b + 1], frm[b]


def build(n, p, recv, flags, outlet):
    p, recv, flags, outlet = (np.asarray(a) for a in (p, recv, flags, outlet))
    recv = recv.astype(np.int64)
    inflow = inflow_table(n, p, recv)
    k = (inflow >= 0).sum(axis=1)
    mand = outlet != LINK_NONE
    term = (flags & TERMINAL) != 0
    extra = mand & ~term                                   # the cell creates a link below its outlet
    breaker = (k != 1) | extra                             # where a link starts: everything else continues the link of its one inflow

    # ---- chains: the nearest breaker strictly upstream of every k == 1 cell and the distance to it, by pointer jumping up the single inflow
    J = np.arange(n)
    one = k == 1
    J[one] = inflow[one].max(axis=1)
    D = np.where(one, 1, 0).astype(np.int64)
    bound = 1
    while (1 << (bound - 1)) < max(n, 1):
        bound += 1
    jump_rounds = 0
    for _ in range(bound):
        go = one & ~breaker[J]
        jump_rounds += 1
        if not go.any():
            break
        D = np.where(go, D + D[J], D)                      # (the right-hand sides read the state before the round)
        J = np.where(go, J[J], J)
    resolved = one & breaker[J]                            # not resolved: a cycle of k == 1 cells

    # ---- the nodes of the link tree and where their inflows come from
    nodes = np.flatnonzero(breaker)
    N = len(nodes)
    nid = np.full(n, -1, np.int64)
    nid[nodes] = np.arange(N)
    src = np.full((N, 8), -1, np.int64)                    # node of the link that arrives through slot m, -1 no inflow, -2 never
    dist = np.zeros((N, 8), np.int64)                      # cells between that node and the inflow cell
    for e, c in enumerate(nodes):
        for m in range(8):
            u = inflow[c, m]
            if u < 0:
                continue
            if breaker[u]:
                src[e, m] = nid[u]
            elif resolved[u]:
                src[e, m], dist[e, m] = nid[J[u]], D[u]
            else:
                src[e, m] = -2

    # ---- levels, leaves first: a node is evaluated in the first round after all its sources
    stamp = np.zeros(N, np.int64)
    nh, nroot, nord, nmag = (np.zeros(N, np.int64) for _ in range(4))
    perm = [None] * N
    level_rounds = 0
    for r in range(1, N + 2):
        level_rounds += 1
        done_now = []
        for e in range(N):
            if stamp[e]:
                continue
            s = [m for m in range(8) if src[e, m] != -1]
            if any(src[e, m] < 0 or not (0 < stamp[src[e, m]] < r) for m in s):
                continue
            if not s:
                nh[e], nroot[e], nord[e], nmag[e], perm[e] = 0, nodes[e], 1, 1, []
            else:
                hr = max((nh[src[e, m]] + dist[e, m], nroot[src[e, m]]) for m in s)
                n_order, frm = [int(nord[src[e, m]]) for m in s], list(s)
                if len(s) >= 2:
                    bubble(n_order, frm)
                    o = n_order[-1] + 1 if n_order[-2] == n_order[-1] else n_order[-1]
                else:
                    o = n_order[0]
                nh[e], nroot[e], nord[e], nmag[e], perm[e] = hr[0] + 1, hr[1], o, sum(int(nmag[src[e, m]]) for m in s), frm
            done_now.append(e)
        if not done_now:
            break
        stamp[done_now] = r
    done = stamp > 0

    # ---- link numbers: the exclusive scan of the links each node creates over the nodes in (h, root) order
    kn = k[nodes]
    body = np.where(kn == 0, 1, np.where(kn >= 2, kn - 1, 0))
    cnt = np.where(done, body + extra[nodes], 0)
    key = np.where(done, (nh << 32) | nroot, np.int64(2**63 - 1))
    order_ = np.argsort(key, kind="stable")
    base = np.zeros(N, np.int64)
    base[order_] = np.cumsum(cnt[order_]) - cnt[order_]
    NL = int(cnt.sum())
    idc = base + cnt - 1                                    # the link that goes on below the node

    L = SimpleNamespace(u1=np.full(NL, -1, np.int64), u2=np.full(NL, -1, np.int64), d=np.full(NL, -1, np.int64), order=np.ones(NL, np.int64),
                        mag=np.ones(NL, np.int64), first=np.zeros(NL, np.int64), dbl=np.zeros(NL, np.int64), cnt=np.ones(NL, np.int64),
                        shapekey=np.zeros(NL, np.uint64))
    label = np.full(n, LINK_NONE, np.int64)
    order = np.zeros(n, np.int64)
    points = []                                            # (link, position, cell) of every point but the links' first cells

    def shape_key(pos, c):
        return np.uint64(((pos + 1) << 32) | (int(outlet[c]) & 0xffffffff))

    # ---- pass 1, per node: the links it creates
    for e in np.flatnonzero(done):
        c, ke, b = nodes[e], int(kn[e]), int(base[e])
        nb = int(body[e])
        again = term[c] or mand[c]                         # append_again on the last body link (k != 1)
        if ke == 0:
            L.first[b] = c
            L.dbl[b] = again
            last = b
        elif ke >= 2:
            frm = perm[e]
            up = lambda a: int(idc[src[e, frm[a]]])  # noqa: E731
            u1 = up(ke - 1)
            for m in range(2, ke + 1):
                a = b + m - 2
                L.u1[a], L.u2[a], L.first[a], L.order[a] = u1, up(ke - m), c, nord[e]
                L.mag[a] = L.mag[u1] if m > 2 else nmag[src[e, frm[ke - 1]]]
                L.mag[a] += nmag[src[e, frm[ke - m]]]
                L.dbl[a] = 1 if m < ke else again
                if m < ke:
                    L.d[a] = a + 1
                u1 = a
            last = b + nb - 1
        else:
            last = int(idc[src[e][src[e] != -1][0]])
        if ke != 1:
            L.cnt[b:b + nb] = 1 + L.dbl[b:b + nb]
            if mand[c]:
                L.shapekey[last] = shape_key(0, c)
        label[c], order[c] = last, nord[e]
        if extra[c]:
            a = b + nb
            L.u1[a], L.first[a], L.order[a], L.mag[a] = last, c, nord[e], nmag[e]
            if ke != 1:
                L.d[last] = a
    # ---- pass 2, per node: the links that end on it
    for e in np.flatnonzero(done):
        c, ke, b = nodes[e], int(kn[e]), int(base[e])
        if ke == 0:
            continue
        for m in range(8):
            if src[e, m] < 0:
                continue
            a = int(idc[src[e, m]])
            pos = int(dist[e, m]) + 1 + int(L.dbl[a])
            points.append((a, pos, c))
            L.cnt[a] += 1                                   # (an integer add: the sum does not depend on the order)
            if ke == 1:
                L.d[a] = b
                L.shapekey[a] = max(L.shapekey[a], shape_key(int(dist[e, m]) + 1, c))
            else:
                frm = perm[e]
                j = frm.index(m)                            # the place of the slot after the bubble passes
                L.d[a] = b + max(ke - 1 - j, 1) - 1
    # ---- pass 3, per cell with one inflow that starts no link
    for c in np.flatnonzero(resolved & ~breaker):
        e = nid[J[c]]
        if not done[e]:
            continue
        a = int(idc[e])
        label[c], order[c] = a, nord[e]
        points.append((a, int(D[c]) + int(L.dbl[a]), c))
        L.cnt[a] += 1
        if mand[c]:
            L.shapekey[a] = max(L.shapekey[a], shape_key(int(D[c]), c))   # the outlet furthest down the link is the last one written
    L.shape = np.where(L.shapekey > 0, (L.shapekey & np.uint64(0xffffffff)).astype(np.uint32).astype(np.int32).astype(np.int64), -1)
    return SimpleNamespace(label=label, order=order, L=L, points=points, n_links=NL, jump_rounds=jump_rounds, level_rounds=level_rounds, nh=nh, nroot=nroot,
                           nodes=nodes, done=done)


def tree_rows(L):
    NL = len(L.cnt)
    rev = np.arange(NL)[::-1]
    cnt = L.cnt[rev]
    beg = np.cumsum(cnt) - cnt
    return np.stack([rev, beg, beg + cnt - 1, L.d[rev], L.u1[rev], L.u2[rev], L.order[rev], L.shape[rev], L.mag[rev]], axis=1).astype(np.int64).reshape(-1, 9)


def rows(model, idx, nx, fel, ad8, length, dxA, dyA, gt):
    L = model.L
    tree = tree_rows(L)
    NL = len(L.cnt)
    beg = np.zeros(NL, np.int64)
    beg[tree[:, 0]] = tree[:, 1]
    coord = np.full((int(L.cnt.sum()), 5), np.nan, np.float64)
    cellarea = np.float64(dxA) * np.float64(dyA)

    def point(row, c):
        x, y = int(idx[c]) % nx, int(idx[c]) // nx
        coord[row] = (gt[0] + gt[1] / 2. + x * gt[1], gt[2] - gt[3] / 2. - y * gt[3], length[c], fel[c], np.float32(np.float64(ad8[c]) * cellarea))

    for a in range(NL):
        point(beg[a], L.first[a])
        if L.dbl[a]:
            point(beg[a] + 1, L.first[a])
    for a, pos, c in model.points:
        point(beg[a] + pos, c)
    assert not np.isnan(coord[:, 0]).any(), "a point of a link was never written"
    return tree, coord


def fifo(n, p, recv, flags, outlet):
    """taudem_amd/csrc/streamnet_links.cpp line by line: (label, order, tree rows, pop order)."""
    inflow = inflow_table(n, np.asarray(p), np.asarray(recv).astype(np.int64))
    waiting = (inflow >= 0).sum(axis=1)
    ident = [int(v) for v in outlet]
    label, order = [LINK_NONE] * n, [0] * n
    queue = [c for c in range(n) if waiting[c] == 0]
    links = []

    def create(u1, u2, c):
        links.append(dict(u1=u1, u2=u2, d=-1, mag=1, shape=-1, first=c, cnt=1, order=1, dbl=0))
        return len(links) - 1

    def again(u):
        links[u]["cnt"] += 1
        links[u]["dbl"] = 1

    head = 0
    while head < len(queue):
        c = queue[head]
        head += 1
        frm = [m for m in range(8) if inflow[c, m] >= 0 and ident[inflow[c, m]] != LINK_NONE]
        n_order = [order[inflow[c, m]] for m in frm]
        k = len(frm)
        mand, term, shape = ident[c] != LINK_NONE, bool(flags[c] & TERMINAL), ident[c]
        if k == 0:
            last, o = create(-1, -1, c), 1
            if not mand and term:
                again(last)
        elif k == 1:
            last = ident[inflow[c, frm[0]]]
            links[last]["cnt"] += 1
            o = n_order[0]
        else:
            bubble(n_order, frm)
            o = n_order[-1] + 1 if n_order[-2] == n_order[-1] else n_order[-1]
            u1 = ident[inflow[c, frm[k - 1]]]
            for m in range(2, k + 1):
                u2 = ident[inflow[c, frm[k - m]]]
                if m == 2:
                    links[u1]["cnt"] += 1
                else:
                    again(u1)
                links[u2]["cnt"] += 1
                nl = create(u1, u2, c)
                links[nl]["order"] = o
                links[nl]["mag"] = links[u1]["mag"] + links[u2]["mag"]
                links[u1]["d"] = links[u2]["d"] = nl
                u1 = nl
            last = u1
            if not mand and term:
                again(last)
        ident[c] = label[c] = last
        order[c] = o
        if mand:
            if k != 1:
                again(last)
            links[last]["shape"] = shape
            if not term:
                nl = create(last, -1, c)
                links[nl]["order"], links[nl]["mag"] = links[last]["order"], links[last]["mag"]
                links[last]["d"] = nl
                ident[c] = nl
        r = int(recv[c])
        if r >= 0 and r != c:
            waiting[r] -= 1
            if waiting[r] == 0:
                queue.append(r)
    L = SimpleNamespace(**{f: np.array([ln[f] for ln in links], np.int64) for f in ("u1", "u2", "d", "mag", "shape", "first", "cnt", "order", "dbl")})
    return np.array(label, np.int64), np.array(order, np.int64), tree_rows(L), queue
