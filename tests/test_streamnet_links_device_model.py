"""The device link builder's definition (tests/streamnet_links_device_model.py: (h, root) by levels, link numbers by a scan over the sorted creating
cells, chains by pointer jumping - no queue) against the reference's -tree and -coord bytes on every golden case and every hand-built raster, and against
the host builder's literal FIFO on random forests with shuffled indices.  CPU only."""
import os

import numpy as np
import pytest

import streamnet_links_device_model as D
import streamnet_model as M


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    d = tmp_path_factory.mktemp("streamnet_links_device_model")
    return M.compile(d), d


def model_files(restate, tag, p, src, fel, ad8, dxc, dyc, gt, outlets, sw):
    rs, d = restate
    dump = os.path.join(str(d), tag + ".bin")
    rs.run(p, src, fel, ad8, dxc, dyc, gt, *outlets, sw=sw, dump=dump)
    ny, nx = p.shape
    dxa = abs(float(np.broadcast_to(np.asarray(dxc, np.float64), (ny,))[ny // 2]))
    dya = abs(float(np.broadcast_to(np.asarray(dyc, np.float64), (ny,))[ny // 2]))
    c = D.read_compact(dump)
    m = D.build(c.n, c.p, c.recv, c.flags, c.outlet)
    tree, coord = D.rows(m, c.idx, nx, c.fel, c.ad8, c.len, dxa, dya, gt)
    return M.tree_text(tree).encode(), M.coord_text(coord).encode()


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", M.CASES)
def test_cases_equal_reference(restate, name, variant):
    g = M.load_golden(name)
    c = M.case_fields(name)
    o = (g["cols"], g["rows"], g["ids"]) if variant == "outlets" else ((), (), ())
    tree, coord = model_files(restate, f"{name}_{variant}", g["p"], g["src"], c["fel"], c["ad8"], c["dxc"], c["dyc"], M.gt4(g["gt"]), o, variant == "sw")
    assert tree == bytes(g["tree_" + variant]), "-tree differs"
    assert coord == bytes(g["coord_" + variant]), "-coord differs"


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", sorted(M.small_rasters()))
def test_hand_built_equal_reference(restate, name, variant):
    g = M.load_golden("small")
    p, src = M.small_rasters()[name]
    fel, ad8 = M.small_fields(p)
    o = M.SMALL_OUTLETS if variant == "outlets" else ((), (), ())
    tree, coord = model_files(restate, f"{name}_{variant}", p, src, fel, ad8, M.SMALL_DX, M.SMALL_DY, M.gt4(M.SMALL_GT), o, variant == "sw")
    assert tree == bytes(g[f"{name}_tree_{variant}"]), "-tree differs"
    assert coord == bytes(g[f"{name}_coord_{variant}"]), "-coord differs"


def random_forest(rng, n):
    """A forest of n nodes with fan-in up to 7 and shuffled indices: every child sits in a slot of its own at its parent; some nodes are terminal, some
    carry an outlet, and now and then two nodes point at each other."""
    name = rng.permutation(n)
    recv = np.full(n, -1, np.int64)
    p = np.zeros(n, np.int16)
    free = {}
    for i in range(1, n):
        if rng.random() < 0.08:
            continue                                        # another root
        for _ in range(4):
            parent = int(rng.integers(0, i))
            slots = free.setdefault(parent, list(rng.permutation(8)))
            if len(slots) > 1:                              # fan-in up to 7
                recv[name[i]] = name[parent]
                p[name[i]] = (int(slots.pop()) + 4) % 8 + 1   # slot (k - 1 + 4) % 8
                break
    if n >= 6 and rng.random() < 0.3:                       # the last node and its receiver point at each other: nothing on the cycle pops
        b = name[n - 1]
        a = recv[b]
        if a >= 0:
            slots = free.setdefault(n - 1, list(rng.permutation(8)))
            recv[a], p[a] = b, (int(slots.pop()) + 4) % 8 + 1
    flags = (rng.random(n) < 0.15).astype(np.uint8)
    outlet = np.where(rng.random(n) < 0.12, rng.integers(-5, 1000, n), D.LINK_NONE).astype(np.int32)
    return p, recv, flags, outlet


def test_closed_form_equals_the_fifo_on_random_forests():
    rng = np.random.default_rng(20261)
    deepest = 0
    for trial in range(300):
        n = int(rng.integers(1, 401))
        p, recv, flags, outlet = random_forest(rng, n)
        label, order, tree, queue = D.fifo(n, p, recv, flags, outlet)
        m = D.build(n, p, recv, flags, outlet)
        assert np.array_equal(m.label, label) and np.array_equal(m.order, order), f"trial {trial}: labels or orders differ"
        assert np.array_equal(D.tree_rows(m.L), tree), f"trial {trial}: link rows differ"
        # the pop order of the cells where links start is the ascending order of (h, root)
        popped = [c for c in queue if c in set(m.nodes[m.done].tolist())]
        by_key = sorted(np.flatnonzero(m.done), key=lambda e: (m.nh[e], m.nroot[e]))
        assert popped == [int(m.nodes[e]) for e in by_key], f"trial {trial}: pop order"
        deepest = max(deepest, m.level_rounds)
    assert deepest >= 5


def test_jump_rounds_of_a_long_chain():
    n = 4096
    recv = np.append(np.arange(1, n), -1)
    p = np.full(n, 1, np.int16)
    m = D.build(n, p, recv, np.zeros(n, np.uint8), np.full(n, D.LINK_NONE, np.int32))
    assert m.n_links == 1 and m.L.cnt[0] == n and m.jump_rounds >= 12 and m.level_rounds == 2
