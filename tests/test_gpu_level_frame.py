"""The frame around the sweeps of a level-field tile activation (flats.hpp: LevelPlainT, tile_relax.hpp: relax_tile_reg).

Plain tiles read no mask byte: whether a cell may move is in its marker alone, and the incrise mask raster exists only for the forms that still
decode it (TDX_FLATS_MASKED=1 and the LDS / worklist hooks).  The first half holds that to seeded DEMs and to hand-built rasters whose in-queue
cells have an EMPTY mask - level-2 quirk seeds, a one-cell pit, a lone flat cell beside a lake - in every form of the classification and of the
operator.  The second half is about the activation flags of the write-back: one-cell-wide canals whose levels count up from an outlet through
every side and every corner of the middle tile (a dropped flag leaves the upper end unresolved), the same paths as trenches that PitRemove
has to fill to their sills, with and without the activation filter, and under a 65 / 64 / 63-row strip cut.  Everything is bit for bit against
the restatement."""
import numpy as np
import pytest

from conftest import bits_equal, describe_diff

pytestmark = pytest.mark.gpu
FEL_ND = -3.0e38


def _slope(shape, ax, ay):
    """A plane without flats: integer steps ax / ay per column / row (|ax| != |ay|, so no two neighbours are level)."""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return (100000.0 + ax * xx + ay * yy).astype(np.float32)


def _plane(shape):
    return np.full(shape, 100.0, dtype=np.float32)


def _pit(shape):
    z = _slope(shape, -17.0, -16.0)
    z[100, 100] -= 50.0   # below all eight neighbours, never filled: in the queue, no neighbour in the queue
    return z


def _lake(z, y0, y1, x0, x1):
    z[y0:y1, x0:x1] = z[y0:y1, x0:x1].min()   # level with its lowest corner, which drains


def _ringed_beside_lake(shape):
    z = _slope(shape, -17.0, -16.0)
    _lake(z, 70, 111, 70, 121)
    z[90, 122] -= 50.0    # one column off the shore, same tile (64 .. 127): ringed by higher ground, above the lake
    return z


def _lake_with_island(shape):
    z = _slope(shape, -17.0, -16.0)
    island = z[90:101, 90:101].copy()
    _lake(z, 40, 151, 40, 151)   # the whole middle tile and a margin of all eight tiles around it
    z[90:101, 90:101] = island
    return z


# name -> (shape, path as (rows, columns) with the OUTLET LAST, ax, ay): the plane falls along the path, so every cell of the path but the last
# few lies below its walls and level with the outlet
def _paths():
    i = np.arange(151)
    d = np.arange(131)
    P = {
        "side_drains_east": ((192, 192), (np.full(151, 96), 20 + i), -17.0, -1.0),
        "side_drains_west": ((192, 192), (np.full(151, 96), 170 - i), 17.0, -1.0),
        "side_drains_south": ((192, 192), (20 + i, np.full(151, 96)), -1.0, -17.0),
        "side_drains_north": ((192, 192), (170 - i, np.full(151, 96)), -1.0, 17.0),
        # (63, 63) -> (64, 64) and (127, 127) -> (128, 128); the anti-diagonal through (63, 128) -> (64, 127) and (127, 64) -> (128, 63)
        "corner_drains_se": ((192, 192), (30 + d, 30 + d), -17.0, -16.0),
        "corner_drains_nw": ((192, 192), (160 - d, 160 - d), 17.0, 16.0),
        "corner_drains_sw": ((192, 192), (30 + d, 161 - d), 17.0, -16.0),
        "corner_drains_ne": ((192, 192), (160 - d, 31 + d), -17.0, 16.0),
        "edge_row_63": ((192, 192), (np.full(151, 63), 20 + i), -17.0, -1.0),
        "edge_row_64": ((192, 192), (np.full(151, 64), 20 + i), -17.0, -1.0),
        "edge_col_63": ((192, 192), (20 + i, np.full(151, 63)), -1.0, -17.0),
        "edge_col_64": ((192, 192), (20 + i, np.full(151, 64)), -1.0, -17.0),
        # 600 cells through ten tiles, one cell per sweep: every tile yields at its sweep cap again and again while its right-hand neighbour waits
        "long_drains_west": ((64, 640), (np.full(600, 32), 619 - np.arange(600)), 17.0, -1.0),
    }
    return P


PATHS = _paths()
CORNERS = [n for n in PATHS if n.startswith("corner_")]


def _canal(name, trench=False):
    """The path as a level canal (a flat for the flow directions), or as a trench whose floor RISES towards the outlet (a pit that fills to the sill)."""
    shape, (ys, xs), ax, ay = PATHS[name]
    z = _slope(shape, ax, ay)
    sill = z[ys[-1], xs[-1]]
    assert (z[ys, xs] >= sill).all()
    n = len(ys)
    z[ys, xs] = sill - (np.float32(0.25) * np.arange(n - 1, -1, -1, dtype=np.float32) if trench else np.float32(0.0))
    return z


HAND = {"plane": lambda: _plane((193, 200)), "pit": lambda: _pit((192, 192)), "ringed_beside_lake": lambda: _ringed_beside_lake((193, 200)),
        "lake_with_island": lambda: _lake_with_island((192, 192))}
SEEDED = {"seeded_257x301": ((257, 301), 5), "seeded_200x333": ((200, 333), 6)}
FORMS = [{}, {"TDX_FLATS_MACRO": "0"}, {"TDX_FLATS_LIST": "1"}, {"TDX_LEVELS_INT32": "1"}, {"TDX_FLATS_MASKED": "1"}, {"TDX_FLATS_MASKED": "2"}, {"TDX_FLATS_FUSED": "1"}]
_cache = {}


def _fel(oracle, name):
    """The pit-filled raster `name` and the restatement's directions of it, computed once."""
    if name not in _cache:
        if name in HAND:
            fel = HAND[name]()
        elif name in SEEDED:
            fel = oracle.pitremove(oracle.synth_dem(*SEEDED[name]), -9999.0)
        else:
            fel = _canal(name)
        p_o, sd8_o, st_o = oracle.d8flowdir(fel, FEL_ND, 30.0, 30.0)
        ang_o, slp_o = oracle.dinfflowdir(fel, FEL_ND, 30.0, 30.0)[:2]
        if name in PATHS:
            assert st_o["flats_initial"] >= len(PATHS[name][1][0]) - 4, "the canal is one flat"
        _cache[name] = (fel, p_o, sd8_o, ang_o, slp_o, st_o)
    return _cache[name]


def _filled_trench(oracle, name):
    """The restatement's PitRemove of the trench `name`, computed once: level from its far end to the sill (a wall cell beside the outlet may spill first)."""
    if ("trench", name) not in _cache:
        dem = _canal(name, trench=True)
        fel_o = oracle.pitremove(dem, -9999.0)
        ys, xs = PATHS[name][1]
        assert (fel_o[ys[:-8], xs[:-8]] == fel_o[ys[0], xs[0]]).all() and fel_o[ys[0], xs[0]] > dem[ys[-8], xs[-8]], "the trench fills through every crossing"
        _cache[("trench", name)] = (dem, fel_o)
    return _cache[("trench", name)]


def _check_directions(ctx, oracle, name, what):
    fel, p_o, sd8_o, ang_o, slp_o, st_o = _fel(oracle, name)
    p, sd8, st = ctx.d8flowdir(fel, FEL_ND, 30.0, 30.0, stats=True)
    assert bits_equal(p, p_o), describe_diff(p, p_o, f"{name} {what}: p")
    assert bits_equal(sd8, sd8_o), describe_diff(sd8, sd8_o, f"{name} {what}: sd8")
    assert st["flats_initial"] == st_o["flats_initial"] and st["flat_iterations"] == st_o["flat_iterations"] and st["flats_left"] == st_o["flats_left"], (name, what, st, st_o)
    ang, slp = ctx.dinfflowdir(fel, FEL_ND, 30.0, 30.0)[:2]
    assert bits_equal(ang, ang_o), describe_diff(ang, ang_o, f"{name} {what}: ang")
    assert bits_equal(slp, slp_o), describe_diff(slp, slp_o, f"{name} {what}: slp")


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "-".join(f"{k[4:].lower()}{v}" for k, v in f.items()) or "default")
@pytest.mark.parametrize("name", list(SEEDED) + list(HAND))
def test_plain_tiles_read_no_mask(name, form, ctx, oracle, monkeypatch):
    """Cells with an empty mask are left alone by the operator itself, on every form (the two TDX_FLATS_MASKED forms still use the rasters)."""
    for k, v in form.items():
        monkeypatch.setenv(k, v)
    _check_directions(ctx, oracle, name, str(form))


def test_hand_built_rasters_are_what_they_claim(oracle):
    """The pit is a flat queue of one cell, the lone cell is in the queue beside its lake, the plane and the lake are flats."""
    assert _fel(oracle, "pit")[5]["flats_initial"] == 1 and _fel(oracle, "ringed_beside_lake")[5]["flats_initial"] > 41 * 51 - 2 * (41 + 51)
    assert _fel(oracle, "plane")[5]["flats_initial"] > 191 * 198 - 1 and _fel(oracle, "lake_with_island")[5]["flats_initial"] > 111 * 111 - 11 * 11 - 4 * 111


@pytest.mark.parametrize("form", [{}, {"TDX_FLATS_LIST": "1"}], ids=["stream", "list"])
def test_second_call_sees_nothing_of_the_first(form, ctx, oracle, monkeypatch):
    """Two calls in a row on one context, the second with fewer flats: no marker or mask of the first call's rasters reaches the second."""
    for k, v in form.items():
        monkeypatch.setenv(k, v)
    for name in ("lake_with_island", "pit", "seeded_200x333", "ringed_beside_lake", "plane", "pit"):
        _check_directions(ctx, oracle, name, f"after the previous raster, {form}")


@pytest.mark.parametrize("filter_off", [False, True], ids=["filter", "every-rim-cell"])
@pytest.mark.parametrize("name", list(PATHS))
def test_canal_levels_cross_every_side_and_corner(name, filter_off, ctx, oracle, monkeypatch):
    if filter_off:
        monkeypatch.setenv("TDX_ACT_FILTER_OFF", "1")
    _check_directions(ctx, oracle, name, f"filter_off={filter_off}")


@pytest.mark.parametrize("no_coarse", [False, True], ids=["coarse", "no-coarse"])
@pytest.mark.parametrize("filter_off", [False, True], ids=["filter", "every-rim-cell"])
@pytest.mark.parametrize("name", list(PATHS))
def test_trench_fills_to_its_sill(name, filter_off, no_coarse, ctx, oracle, monkeypatch):
    if filter_off:
        monkeypatch.setenv("TDX_ACT_FILTER_OFF", "1")
    if no_coarse:
        monkeypatch.setenv("TDX_PIT_NO_COARSE", "1")
    dem, fel_o = _filled_trench(oracle, name)
    fel = ctx.pitremove(dem, -9999.0)
    assert bits_equal(fel, fel_o), describe_diff(fel, fel_o, f"{name} filter_off={filter_off} no_coarse={no_coarse}: fel")


@pytest.mark.parametrize("name", ["lake_with_island"] + CORNERS)
def test_strips_of_65_64_63_rows_equal_one_gpu(name, ctx, oracle):
    """The strip form of tests/test_gpu_fuzz_strips.py on a cut that puts no strip boundary on a tile boundary of the 192-row raster."""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline

    dem = HAND[name]() if name in HAND else _canal(name, trench=True)
    ny, nx = dem.shape
    assert ny == 192
    fel1 = ctx.pitremove(dem, -9999.0)
    p1, sd81 = ctx.d8flowdir(fel1, FEL_ND, 30.0, 30.0)
    ang1, slp1 = ctx.dinfflowdir(fel1, FEL_ND, 30.0, 30.0)[:2]
    parts = [(0, 65), (65, 129), (129, 192)]
    with StripGroup(len(parts), nx, [0] * len(parts)) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            nyl = y1 - y0
            pipe = StripPipeline(c, comm, nx, nyl)
            sl = slice(1, nyl + 1)
            d = pipe.empty(torch.float32)
            d[sl] = torch.from_numpy(np.ascontiguousarray(dem[y0:y1])).cuda()
            fel, _ = pipe.pitremove(d, -9999.0)
            p, sd8, _ = pipe.d8flowdir(fel, FEL_ND, 30.0, 30.0)
            ang, slp, _ = pipe.dinfflowdir(fel, FEL_ND, 30.0, 30.0)
            return {k: v[sl].cpu().numpy() for k, v in (("fel", fel), ("p", p), ("sd8", sd8), ("ang", ang), ("slp", slp))}
        res = grp.run(rank_main)
    for key, ref in (("fel", fel1), ("p", p1), ("sd8", sd81), ("ang", ang1), ("slp", slp1)):
        got = np.concatenate([r[key] for r in res], axis=0)
        assert bits_equal(got, ref), describe_diff(got, ref, f"{name} in strips of 65 / 64 / 63 rows: {key}")
