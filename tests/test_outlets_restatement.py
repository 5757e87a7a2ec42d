"""The restatement of MoveOutletsToStrm and ConnectDown (tests/outlets/outlets_restate.c through tests/outlets_model.py) against the goldens of the
real tools (tests/golden/outlets_*.npz, written by tests/golden/make_golden_outlets.py): coordinates to the bit and fields as text, which is what
the recorded lines hold.  And against itself under every cut into row strips, in a CPU model of the hand-over.  No GPU is needed."""
import numpy as np
import pytest

import outlets_model as M


@pytest.fixture(scope="module")
def R(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("outlets_restate"))


def _move(R, p, src, gt, g, md, prefix=""):
    cols, rows = M.to_cells(gt, g[prefix + "ox"], g[prefix + "oy"])
    rx, ry, d = R.moveoutlets(p, src, cols, rows, md)
    return M.move_record(gt, g[prefix + "ox"], g[prefix + "oy"], g[prefix + "ids"], rx, ry, d)


@pytest.mark.parametrize("name", M.CASES)
def test_cases_equal_the_reference(R, name):
    p, src, w, ad8, gt, _ = M.inputs(name)
    g = M.load_golden(name)
    cols, rows = M.to_cells(gt, g["ox"], g["oy"])
    M.check_outlet_points(p, src, cols, rows)
    assert M.tied_watersheds(w, ad8)
    for md in M.MAXDISTS:
        assert _move(R, p, src, gt, g, md) == bytes(g[f"move_md{md}"]), f"{name}: -md {md}"
    for dd in M.MOVEDISTS:
        o, od = M.connect_records(gt, R.connectdown(p, w, ad8, dd))
        assert o == bytes(g[f"connect_o_d{dd}"]) and od == bytes(g[f"connect_od_d{dd}"]), f"{name}: -d {dd}"


def test_the_kinds_of_outlets_end_as_the_issue_says(R):
    """on the stream 0; one cell off 1; the far one -1 under -md 3; p = 0, off the raster edge, nodata of p: -1 with the original coordinates"""
    p, src, w, ad8, gt, _ = M.inputs("plain")
    g = M.load_golden("plain")
    rows3 = M.parse_record(g["move_md3"])
    rows50 = M.parse_record(g["move_md50"])
    k = {n: i for i, n in enumerate(M.OUTLET_KINDS)}
    d3 = [int(r[2]["Dist_moved"]) for r in rows3]
    d50 = [int(r[2]["Dist_moved"]) for r in rows50]
    assert d3[k["on_stream"]] == 0 and d3[k["one_off"]] == 1 and d3[k["far"]] == -1 and d50[k["far"]] > 3
    for n in ("ends_in_p0", "leaves_raster", "p_nodata", "off_raster"):
        assert d50[k[n]] == -1 and (rows50[k[n]][0], rows50[k[n]][1]) == (float(g["ox"][k[n]]), float(g["oy"][k[n]])), n
    assert d50[k["twice_a"]] == d50[k["twice_b"]] == 2 and rows50[k["twice_a"]][:2] == rows50[k["twice_b"]][:2]
    assert [r[2]["id"] for r in rows50] == [str(int(i)) for i in g["ids"]]


def test_hand_built_rasters_equal_the_reference(R):
    g = M.load_golden("small")
    rasters = M.small_rasters()
    assert list(g["names"]) == list(rasters)
    for name, (p, w, ad8) in rasters.items():
        src = M.small_src(w, ad8)
        for md in M.MAXDISTS:
            assert _move(R, p, src, M.SMALL_GT, g, md, name + "_") == bytes(g[f"{name}_move_md{md}"]), f"{name}: -md {md}"
        for dd in M.MOVEDISTS:
            res = R.connectdown(p, w, ad8, dd)
            if int(g[f"{name}_nopoints"]):
                assert name == "all_nodata" and res[0].size == 0
                continue
            o, od = M.connect_records(M.SMALL_GT, res)
            assert o == bytes(g[f"{name}_connect_o_d{dd}"]) and od == bytes(g[f"{name}_connect_od_d{dd}"]), f"{name}: -d {dd}"


def test_hand_built_rasters_hold_what_they_are_for(R):
    r = M.small_rasters()
    ids, x, y, amax, *_ = R.connectdown(*r["tie_far_apart"][:1], r["tie_far_apart"][1], r["tie_far_apart"][2], 0)
    assert list(ids) == [6, 7] and (x[0], y[0]) == (5, 2) and (38 * 64 + 5) - (2 * 64 + 5) > 2048 and (x[1], y[1]) == (40, 20)
    ids, x, y, amax, *_ = R.connectdown(r["tie_in_one_wave"][0], r["tie_in_one_wave"][1], r["tie_in_one_wave"][2], 0)
    assert (x[0], y[0]) == (17, 0)
    ids, x, y, amax, *_ = R.connectdown(r["minus_zero"][0], r["minus_zero"][1], r["minus_zero"][2], 0)
    assert [(int(a), int(b)) for a, b in zip(x, y)] == [(3, 0), (3, 2)] and np.signbit(amax[0]) and not np.signbit(amax[1])
    ids, x, y, amax, *_ = R.connectdown(r["nan_first_and_later"][0], r["nan_first_and_later"][1], r["nan_first_and_later"][2], 0)
    assert (x[0], y[0]) == (0, 0) and np.isnan(amax[0]) and (x[1], y[1], amax[1]) == (2, 3, 6.0)
    ids, x, y, amax, *_ = R.connectdown(r["nan_heads_a_strip"][0], r["nan_heads_a_strip"][1], r["nan_heads_a_strip"][2], 0)
    assert (x[0], y[0], amax[0]) == (3, 2, 10.0) and (x[1], y[1]) == (5, 0) and np.isnan(amax[1])      # the NaN that heads row 2 is passed over, the one that heads id 2 stands
    ids, *_ = R.connectdown(r["largest_id_last_cell"][0], r["largest_id_last_cell"][1], r["largest_id_last_cell"][2], 0)
    assert list(ids) == [1, 40]
    g = M.load_golden("small")
    far = [int(row[2]["Dist_moved"]) for row in M.parse_record(g["long_row_move_md50"])]
    # outlets on columns 0, 3, ... 69, the only stream cell on column 68: 68 .. 53 steps are too many, 50 are not; column 69 walks off the raster
    assert far[:6] == [-1] * 6 and far[6] == 50 and far[22] == 2 and far[23] == -1 and max(far) == 50


def test_refusals(R):
    p, w, ad8 = (a.copy() for a in M.small_rasters()["id_zero"])
    w[1, 1] = -4
    with pytest.raises(ValueError):
        R.connectdown(p, w, ad8, 2)
    w[1, 1] = 50
    with pytest.raises(ValueError):
        R.connectdown(p, w, ad8, 2, cap=49)
    assert R.connectdown(p, w, ad8, 2, cap=50)[0].max() == 50


def _cuts(ny, rng, k):
    return sorted(int(v) for v in rng.choice(np.arange(1, ny), size=min(k, ny - 1), replace=False))


@pytest.mark.parametrize("name", M.CASES)
def test_any_cut_into_strips_gives_the_one_rank_result(R, name):
    p, src, w, ad8, gt, _ = M.inputs(name)
    ny, nx = p.shape
    rng = np.random.default_rng(sum(name.encode()))
    cells = rng.choice(p.size, 300, replace=False)
    cols, rows = (cells % nx).astype(np.int32), (cells // nx).astype(np.int32)
    for k in (1, 2, 5, ny - 1):
        cuts = _cuts(ny, rng, k)
        for md in (50, 3):
            want = R.moveoutlets(p, src, cols, rows, md)
            got = R.moveoutlets_strips(p, src, cols, rows, md, cuts)
            assert all(np.array_equal(a, b) for a, b in zip(want, got[:3])), (name, cuts, md)
        for dd in (10, 2):
            want = R.connectdown(p, w, ad8, dd)
            got = R.connectdown_strips(p, w, ad8, dd, cuts)
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(want, got[:7])), (name, cuts, dd)


def zigzag(ny=12, nx=9, cut=6):
    """A path that crosses the cut between rows cut - 1 and cut four times before it meets the stream; returns p, src, the start cell."""
    p = np.full((ny, nx), 1, np.int16)
    src = np.zeros((ny, nx), np.int32)
    y, x = cut - 1, 0
    for d in (8, 2, 8, 2):          # SE, NE, SE, NE: down, up, down, up over the cut
        p[y, x] = d
        y, x = y + M.DY_[d], x + M.DX_[d]
    src[y, x] = 1
    return p, src, (0, cut - 1)


def test_a_path_that_crosses_one_cut_four_times(R):
    p, src, (c0, r0) = zigzag()
    want = R.moveoutlets(p, src, [c0], [r0], 50)
    assert want[2][0] == 4
    got = R.moveoutlets_strips(p, src, [c0], [r0], 50, [6])
    assert all(np.array_equal(a, b) for a, b in zip(want, got[:3])) and got[3] >= 3     # several rounds: the outlet came back
    w = np.ones_like(src); w[:6] = 2
    ad8 = np.zeros(p.shape, np.float32); ad8[r0, c0] = 9
    a = R.connectdown(p, w, ad8, 7)
    b = R.connectdown_strips(p, w, ad8, 7, [6])
    assert all(np.array_equal(u, v) for u, v in zip(a, b[:7])) and b[7] >= 3


def test_every_row_a_strip_on_the_hand_built_rasters(R):
    for name, (p, w, ad8) in M.small_rasters().items():
        ny = p.shape[0]
        cuts = list(range(1, ny))
        cols, rows, _ = M.small_outlets(p)
        src = M.small_src(w, ad8)
        want, got = R.moveoutlets(p, src, cols, rows, 3), R.moveoutlets_strips(p, src, cols, rows, 3, cuts)
        assert all(np.array_equal(a, b) for a, b in zip(want, got[:3])), name
        want, got = R.connectdown(p, w, ad8, 2), R.connectdown_strips(p, w, ad8, 2, cuts)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(want, got[:7])), name
