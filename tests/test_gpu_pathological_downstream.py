"""The tools downstream of the flow directions on inputs that are nothing like a fractal surface (tests/pathological.py), one device and
in row strips: DinfUpDependence, DinfRevAccum, DinfDecayAccum, DinfConcLimAccum, DinfTransLimAccum, DinfDistDown, DinfDistUp,
D8HDistToStrm, GageWatershed, GridNet, D8FlowPathExtremeUp and Threshold, each fed the ORACLE's directions so that a difference is
located in the tool itself, each held bit for bit to its pinned restatement (tests/downstream.py), the -id text byte for byte.  The
restatements are held to the reference on reduced versions of these rasters by tests/test_pathological_restatements.py; the GPU is held
to those fixtures directly as well.  Strips of one and two rows: both halo rows belong to neighbours whose only owned row is the one
exchanged (`--gpus 8` on a 5-row raster runs five 1-row ranks, capi_tools.cpp).

The five sweep tools that came later - RetLimFlow, DinfAvalanche, FlowDirCond, D8VDistToStrm, SlopeAveDown - run in the same four settings
in tests of their own (test_late_tools_*: downstream.extras_late / reference_late / single_late / strip_late / compare_late), so that a
failure names the tool and the tests above keep their times.  DinfAvalanche is compared by aval_model.compare_aval; every line it prints
holds the cells with rz data and the tainted share.  The restatement alone, with the sources extras_late chooses (path / -direct at
alpha 18, path / -direct at alpha 1; no tainted cell in any of them):

    ramp_diag       168 /   1,  68 646 /    755   (-direct: one source cell; scattered sources taint 12 - 55 % of a -direct runout)
    ramp_antidiag   170 /   1,  70 084 /  7 132   (the same)
    ramp_x          148 / 148,  14 887 / 14 887        ramp_-x       168 / 168,  16 024 / 16 024
    ramp_y          164 / 164,  13 584 / 13 584        ramp_-y       141 / 141,  11 933 / 11 933
    spiral        2 939 / 3 076,  9 264 /  9 557       nan_cells     210 / 210,   7 065 /  7 401
    +inf_cells      207 / 207,   7 173 /  7 634        -inf_cells    186 / 186,   6 130 /  6 472
    plane 239, ramp_shallow 171, checkerboard_pits 153 in all four (the sources alone: nothing slopes by a degree)
    one_row, one_column, two_rows, one_data_cell, all_nodata: none (every cell is an edge cell without a direction)"""
import time

import numpy as np
import pytest

import downstream as D
import patho_fixture as F
import pathological as P
from cellsizes import rows
from conftest import bits_equal, describe_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R(tmp_path_factory, oracle):
    return D.Restate(tmp_path_factory.mktemp("downstream"), oracle)


def _sizes(i, ny):
    """constant square cells, constant rectangular cells, or `wild` per-row sizes, rotating with i"""
    return [(30.0, 30.0), (10.0, 12.5), rows("wild", ny, seed=i)][i % 3]


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_downstream_on_pathological_input(name, ctx, oracle, R, monkeypatch):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    i = sorted(P.CASES).index(name)
    dem = P.CASES[name](oracle)
    dx, dy = _sizes(i, dem.shape[0])
    inp = D.derive(oracle, dem, dx, dy, 60 + i)
    ref = D.reference(R, inp, dx, dy, i)
    bad = D.compare(D.single(ctx, inp, dx, dy, i), ref, name)
    assert not bad, "\n".join(bad)


def _late_inputs(oracle, R, dem, dx, dy, seed, i, name=None, cut=()):
    """derive() and extras_late() for one raster; a case of tests/pathological.py by `name` runs the avalanche on 30 x 40 cells, with its
    floor and its -direct sources (downstream.LATE_FLOOR / LATE_DIRECT)."""
    inp = D.derive(oracle, dem, dx, dy, seed, cut_rows=cut)
    return D.extras_late(inp, seed, R, dx, dy, i, direct=D.LATE_DIRECT.get(name, "scattered"), floor=D.LATE_FLOOR.get(name, 0), aval_rows=name is None)


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_late_tools_on_pathological_input(name, ctx, oracle, R, monkeypatch):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    i = sorted(P.CASES).index(name)
    dem = P.CASES[name](oracle)
    dx, dy = _sizes(i, dem.shape[0])
    inp = _late_inputs(oracle, R, dem, dx, dy, 60 + i, i, name)
    ref = D.reference_late(R, inp, dx, dy, i)
    bad = D.compare_late(D.single_late(ctx, inp, dx, dy, i), ref, name)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", F.names())
def test_downstream_matches_reference_fixtures(name, ctx, monkeypatch):
    """The GPU against the reference's own rasters on the reduced pathological inputs (tests/golden/make_golden_pathological.py)."""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    g = F.load(name)
    bad = D.compare(F.gpu(ctx, g), F.expected(g), f"patho_{name}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", F.late_names())
def test_late_tools_match_reference_fixtures(name, ctx, R, monkeypatch):
    """The GPU against the reference's own rasters on the reduced pathological inputs (tests/golden/make_golden_patholate.py)."""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    g, inp = F.load_late(name)
    bad = D.compare_late(D.single_late(ctx, inp, F.DX, F.DY, int(g["index"])), F.expected_late(g, R, inp), f"patholate_{name}")
    assert not bad, "\n".join(bad)


def _in_strips(oracle, R, dem, world, dx, dy, i, label):
    """Every strip entry point on `dem` cut into `world` strips (partition_rows), against the restatements on the global rasters:
    the upstream tools from the DEM, the downstream tools from the oracle's directions; gauges and outlets on the cut rows."""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows, strip_rows

    ny, nx = dem.shape
    parts = partition_rows(ny, world)
    cut = sorted({y for y0, y1 in parts for y in (y0 - 1, y0, y1 - 1, y1) if 0 <= y < ny})
    inp = D.derive(oracle, dem, dx, dy, 80 + i, cut_rows=cut)
    ref = dict(D.reference_upstream(oracle, dem, inp, dx, dy), **D.reference(R, inp, dx, dy, i))
    with StripGroup(world, nx, [0] * world) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            nyl = y1 - y0
            pipe = StripPipeline(c, comm, nx, nyl)
            sdx, sdy = strip_rows(dx, y0, y1), strip_rows(dy, y0, y1)

            def put(a):
                t = pipe.empty(getattr(torch, np.asarray(a).dtype.name))
                t[1:nyl + 1] = torch.from_numpy(np.ascontiguousarray(a[y0:y1])).cuda()
                return t
            out = D.strip_upstream(pipe, put, dem, inp, sdx, sdy, y0, y1)
            out.update(D.strip(pipe, put, inp, sdx, sdy, y0, y1, i))
            return out
        res = grp.run(rank_main)
    got = {k: np.concatenate([r[k] for r in res], axis=0) for k in res[0] if k != "gw_id"}
    bad = D.compare(got, {k: v for k, v in ref.items() if k != "gw_id"}, label)
    bad += [f"{label}: rank {r} -id table {res[r]['gw_id']!r} vs {ref['gw_id']!r}" for r in range(world) if res[r]["gw_id"] != ref["gw_id"]]
    assert not bad, "\n".join(bad)


# strips of one and two rows (a halo row on each side that is a neighbour's only owned row), 8 / 5 / 3 ranks of one row, 8 of two rows,
# the pathological two-row raster in two 1-row strips
SHORT = [("8x300 in 8", lambda o: o.synth_dem((8, 300), 71), 8), ("5x130 in 5", lambda o: o.synth_dem((5, 130), 72), 5),
         ("16x257 in 8", lambda o: o.synth_dem((16, 257), 73), 8), ("3x65 in 3", lambda o: o.synth_dem((3, 65), 74), 3),
         ("two_rows in 2", P.CASES["two_rows"], 2)]


@pytest.mark.parametrize("label,make,world", SHORT, ids=[s[0].replace(" ", "_") for s in SHORT])
def test_strips_of_one_and_two_rows(label, make, world, oracle, R, monkeypatch):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    i = [s[0] for s in SHORT].index(label)
    dem = make(oracle)
    dx, dy = _sizes(i, dem.shape[0])
    _in_strips(oracle, R, dem, world, dx, dy, i, label)


def _late_in_strips(oracle, R, dem, world, dx, dy, i, label, name=None):
    """The five late tools' strip entry points on `dem` cut into `world` strips against the restatements on the global rasters."""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows, strip_rows

    ny, nx = dem.shape
    parts = partition_rows(ny, world)
    cut = sorted({y for y0, y1 in parts for y in (y0 - 1, y0, y1 - 1, y1) if 0 <= y < ny})
    inp = _late_inputs(oracle, R, dem, dx, dy, 80 + i, i, name, cut)
    ref = D.reference_late(R, inp, dx, dy, i)
    dns = D.late_dns(dx, dy, i)
    with StripGroup(world, nx, [0] * world) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            nyl = y1 - y0
            pipe = StripPipeline(c, comm, nx, nyl)

            def put(a):
                t = pipe.empty(getattr(torch, np.asarray(a).dtype.name))
                t[1:nyl + 1] = torch.from_numpy(np.ascontiguousarray(a[y0:y1])).cuda()
                return t
            return D.strip_late(pipe, put, inp, strip_rows(dx, y0, y1), strip_rows(dy, y0, y1), y0, y1, ny, dns, i)
        res = grp.run(rank_main)
    bad = D.compare_late({k: np.concatenate([r[k] for r in res], axis=0) for k in res[0]}, ref, label)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("label,make,world", SHORT, ids=[s[0].replace(" ", "_") for s in SHORT])
def test_late_tools_in_strips_of_one_and_two_rows(label, make, world, oracle, R, monkeypatch):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    i = [s[0] for s in SHORT].index(label)
    dem = make(oracle)
    dx, dy = _sizes(i, dem.shape[0])
    _late_in_strips(oracle, R, dem, world, dx, dy, i, label, "two_rows" if label.startswith("two_rows") else None)


@pytest.mark.parametrize("name", ["spiral", "plane", "checkerboard_pits", "nan_cells", "one_data_cell"])
def test_late_tools_pathological_in_three_strips(name, oracle, R, monkeypatch):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    i = sorted(P.CASES).index(name)
    dem = P.CASES[name](oracle)
    _late_in_strips(oracle, R, dem, 3, *_sizes(i, dem.shape[0]), i, f"{name} in 3 strips", name)


@pytest.mark.parametrize("name", ["spiral", "plane", "checkerboard_pits", "nan_cells", "one_data_cell"])
def test_pathological_downstream_in_three_strips(name, oracle, R, monkeypatch):
    """the downstream counterpart of test_gpu_pathological.py::test_pathological_input_in_three_strips"""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    i = sorted(P.CASES).index(name)
    dem = P.CASES[name](oracle)
    _in_strips(oracle, R, dem, 3, *_sizes(i, dem.shape[0]), i, f"{name} in 3 strips")


@pytest.mark.slow
def test_spiral_at_2048_downstream(ctx, oracle, R, capsys):
    """The longest dependency chain the sweeps can meet, for the tools downstream of the directions: a spiral channel at 2048^2 (pitch 8:
    256 windings, a flow path of ~500 k cells).  Every stage is checked on every cell against its restatement; its ms_total / rounds are
    printed.  The first MI355X run took 4.4 s of wall for the first nine stages (0.27 - 0.73 s each, one round each); RetLimFlow,
    FlowDirCond and D8VDistToStrm (its single source at the outlet) are stages ten to twelve; the bound is 60 s, as for
    test_gpu_pathological.py::test_spiral_at_4096_completes."""
    import torch

    dem = P.spiral(2048, 8)
    fel = oracle.pitremove(dem, P.NODATA)
    p, _, _ = oracle.d8flowdir(fel, -3.0e38, 30.0, 30.0)
    ang, _, _ = oracle.dinfflowdir(fel, -3.0e38, 30.0, 30.0)
    ad8 = oracle.aread8(p, -32768, contcheck=False)
    ny, nx = dem.shape
    outlet = np.unravel_index(int(np.argmax(ad8)), ad8.shape)            # the spiral's outlet on the raster edge
    path = np.flatnonzero(ad8.ravel() > 1)
    mid = np.unravel_index(int(path[np.argsort(ad8.ravel()[path])[path.size // 2]]), ad8.shape)   # a channel cell half way up the path
    rng = np.random.default_rng(2048)
    dg = (rng.random((ny, nx)) < 0.001).astype(np.int32)
    w = (0.5 + rng.integers(0, 17, (ny, nx)) / 8.0).astype(np.float32)
    src = np.zeros((ny, nx), np.int32)
    src[outlet] = 1                                                       # one source: the whole channel is one ~500 k-cell path to it
    src16 = src.astype(np.int16)
    gauges = (np.array([outlet[1], mid[1]], np.int32), np.array([outlet[0], mid[0]], np.int32), np.array([7, 3], np.int32))
    sa = (rng.integers(-4, 5, (ny, nx)) * 0.5).astype(np.float32)
    late = np.random.default_rng([2048, 1])                               # (a generator of its own: the draws above keep their bits)
    wg = (late.integers(0, 33, (ny, nx)) / 8.0).astype(np.float32)
    rc = (late.integers(0, 9, (ny, nx)) / 8.0).astype(np.float32)
    z = (fel + np.rint(late.normal(0.0, 3.0, (ny, nx)) * 16.0) / 16.0).astype(np.float32)
    d = f"cuda:{ctx.device}"
    T = {k: torch.from_numpy(np.ascontiguousarray(v)).to(d) for k, v in (("p", p), ("ang", ang), ("fel", fel), ("dg", dg), ("w", w), ("src", src),
                                                                          ("src16", src16), ("sa", sa), ("wg", wg), ("rc", rc), ("z", z))}
    stages = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()

    def run(name, fn):
        out = fn()
        stages.append((name, out[-1]))
        return [o.cpu().numpy() if hasattr(o, "cpu") else o for o in out[:-1]]
    dep, = run("dinfupdependence", lambda: ctx.dinfupdependence(T["ang"], T["dg"], dx=30.0, dy=30.0, stats=True))
    racc, dmax = run("dinfrevaccum", lambda: ctx.dinfrevaccum(T["ang"], T["w"], dx=30.0, dy=30.0, stats=True))
    dd, = run("dinfdistdown ave v", lambda: ctx.dinfdistdown(T["ang"], T["src16"], T["fel"], stat="ave", kind="v", dx=30.0, dy=30.0, stats=True))
    ddh, = run("dinfdistdown min h", lambda: ctx.dinfdistdown(T["ang"], T["src16"], None, stat="min", kind="h", dx=30.0, dy=30.0, stats=True))
    du, = run("dinfdistup", lambda: ctx.dinfdistup(T["ang"], T["fel"], stat="ave", kind="h", dx=30.0, dy=30.0, stats=True))
    dist, = run("d8hdisttostrm", lambda: ctx.d8hdisttostrm(T["p"], T["src"], 1, dx=30.0, dy=30.0, stats=True))
    gw, table = run("gagewatershed", lambda: ctx.gagewatershed(T["p"], gauges, stats=True))
    plen, tlen, gord = run("gridnet", lambda: ctx.gridnet(T["p"], -32768, 30.0, 30.0, stats=True))
    xup, = run("d8flowpathextremeup", lambda: ctx.d8flowpathextremeup(T["p"], T["sa"], -32768, usemax=True, contcheck=False, stats=True))
    qrl, = run("retlimflow", lambda: ctx.retlimflow(T["ang"], T["wg"], T["rc"], dx=30.0, dy=30.0, stats=True))
    zfdc, = run("flowdircond", lambda: ctx.flowdircond(T["p"], T["z"], z_nodata=D.FEL_ND, stats=True))
    vd, = run("d8vdisttostrm", lambda: ctx.d8vdisttostrm(T["p"], T["fel"], T["src"], 1, src_nodata=D.SRC_ND, stats=True))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    with capsys.disabled():
        print("\nspiral 2048^2 downstream: " + ", ".join(f"{k} {s['ms_total']:.1f} ms / {s['rounds']} rounds" for k, s in stages) + f"; wall {wall:.2f} s")
    assert wall < 60.0
    o = oracle
    checks = [("dep", dep, o.dinfupdependence(ang, dg, dx=30.0, dy=30.0))]
    racc_o, dmax_o = o.dinfrevaccum(ang, w, dx=30.0, dy=30.0)
    checks += [("racc", racc, racc_o), ("dmax", dmax, dmax_o)]
    checks += [("dd ave v", dd, R.dd(ang, src16, fel, stat="ave", kind="v", dxc=30.0, dyc=30.0)),
               ("dd min h", ddh, R.dd(ang, src16, None, stat="min", kind="h", dxc=30.0, dyc=30.0)),
               ("du ave h", du, R.du(ang, fel, stat="ave", kind="h", dxc=30.0, dyc=30.0)),
               ("dist", dist, R.rev.dist(p, src, 1, 30.0, 30.0, src_nodata=D.SRC_ND))]
    gw_o, text_o = R.rev.gage(p, *gauges)
    checks.append(("gw", gw, gw_o))
    pl_o, tl_o, go_o = o.gridnet(p, -32768, 30.0, 30.0)
    checks += [("plen", plen, pl_o), ("tlen", tlen, tl_o), ("gord", gord, go_o)]
    checks.append(("xup", xup, o.d8flowpathextremeup(p, sa, -32768, usemax=True, contcheck=False)))
    checks += [("qrl", qrl, R.aval.retlimflow(ang, wg, rc, dxc=30.0, dyc=30.0)), ("zfdc", zfdc, R.last.flowdircond(p, z, D.FEL_ND)),
               ("vd", vd, R.last.vdist(p, fel, src, 1, src_nodata=D.SRC_ND))]
    bad = [describe_diff(a, b, f"spiral 2048^2: {k}") for k, a, b in checks if not bits_equal(a, b)]
    import d8rev_model

    if d8rev_model.table_text(table) != text_o:
        bad.append(f"spiral 2048^2: -id text {d8rev_model.table_text(table)!r} vs {text_o!r}")
    assert not bad, "\n".join(bad)
    assert float(dist.max()) > 30.0 * 4e5, "the single source should lie at the end of a path of ~500 k cells"
