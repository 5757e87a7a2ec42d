"""The SINMAP parameter region grid on the GPU (Context.regiongrid, bin/siregiontool) against the model (tests/regiongrid_model.py): the int16 grid and
the ids are equal exactly, from numpy and from a device out=.

Rasters 1 x 1, 1 x 37, 41 x 1, 5 x 67, 33 x 65 and 70 x 300: narrower than one bitmap word, not word multiples, more than one block of the streaming
pass.  Inputs: the hand cases of test_regiongrid_model.py scaled to the raster, a polygon larger than the raster on all four sides, polygons wholly
off it, a triangle with an edge across all rows, 40 random polygons in a UTM-sized frame with both signs of gt[5] and repeated values, and 3 000
unit squares under a workspace bound of two features (many batches).  The round trip polygonize -> layer file -> read_polygons -> regiongrid gives
the watershed grid back."""
import os
import subprocess

import numpy as np
import pytest
import torch

import regiongrid_model as M
import taudem_amd as T
from taudem_amd import api
from test_gpu_polygonize import GRIDS
from test_regiongrid_model import HAND_CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")
SHAPES = [(1, 1), (1, 37), (41, 1), (5, 67), (33, 65), (70, 300)]
IDENT = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
UTM = {"north_up_30": (4.1e5, 30.0, 0.0, 4.6e6, 0.0, -30.0), "south_up_10x25": (4.1e5, 10.0, 0.0, 4.6e6, 0.0, 25.0)}


def world(gt, ring):
    return [(gt[0] + px * gt[1], gt[3] + py * gt[5]) for px, py in ring]


def hand_scene(shape):
    """Every hand case stretched from its own raster onto this one: one scene per case."""
    ny, nx = shape
    scenes = []
    for _, (hshape, features, values, _) in sorted(HAND_CASES.items()):
        sx, sy = nx / hshape[1], ny / hshape[0]
        scenes.append(([[[(x * sx, y * sy) for x, y in ring] for ring in f] for f in features], values))
    return scenes


def big_scene(shape):
    ny, nx = shape
    around = [(-5.3, -4.2), (nx + 7.7, -3.1), (nx + 3.3, ny + 6.6), (-8.8, ny + 2.2)]            # the raster lies inside: every crossing is off it
    dent = [(-3.0, -2.0), (nx + 4.0, -2.5), (nx * 0.5, ny * 0.5), (nx + 2.0, ny + 3.0), (-6.0, ny + 1.5)]   # crossings left of column 0 and on the raster
    return [([[around]], [4]), ([[dent]], [5]), ([[around], [dent]], [1, 2])]


def off_scene(shape):
    ny, nx = shape
    boxes = [[(nx + 5.0, ny + 5.0), (nx + 20.0, ny + 5.0), (nx + 20.0, ny + 30.0), (nx + 5.0, ny + 30.0)],       # right of and below it
             [(-30.0, 0.2), (-2.0, 0.2), (-2.0, ny - 0.2), (-30.0, ny - 0.2)],                                   # left of it, across its rows
             [(nx + 1.0, -3.0), (nx + 9.0, -3.0), (nx + 9.0, ny + 3.0), (nx + 1.0, ny + 3.0)],                   # right of it, across its rows
             [(0.2, -9.0), (nx - 0.2, -9.0), (nx - 0.2, -1.0), (0.2, -1.0)]]                                     # above it
    return [([[b] for b in boxes], [1, 2, 3, 4])]


def triangle_scene(shape):
    ny, nx = shape
    return [([[[(0.3, -1.0), (nx * 0.9, ny + 1.0), (nx * 0.2, ny + 1.0)]]], [6])]


def random_scene(shape, gt, seed=5):
    """40 polygons of 3 .. 60 vertices around the raster, values 1 .. 5 with repeats: overlaps, self-intersections, the layer order."""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    features, values = [], []
    for _ in range(40):
        n = int(rng.integers(3, 61))
        cx, cy = rng.uniform(-0.1, 1.1) * nx, rng.uniform(-0.1, 1.1) * ny
        ang = np.sort(rng.uniform(0, 2 * np.pi, n)) if rng.random() < 0.7 else rng.uniform(0, 2 * np.pi, n)   # star-shaped, or any vertex order
        rad = rng.uniform(0.05, 0.6, n)
        ring = [(cx + r * nx * np.cos(a), cy + r * ny * np.sin(a)) for a, r in zip(ang, rad)]
        if rng.random() < 0.3:
            ring = [(round(x * 2) / 2, round(y * 2) / 2) for x, y in ring]        # vertices on cell centres and cell corners
        features.append([world(gt, ring)])
        values.append(int(rng.integers(1, 6)))
    return features, values


def check(ctx, shape, gt, features, values, **kw):
    want, want_ids = M.polygons(shape, gt, features, values)
    grid, ids = ctx.regiongrid(shape, gt, polygons=features, values=values, **kw)
    assert grid.dtype == np.int16 and np.array_equal(grid, want), np.argwhere(grid != want)[:5]
    assert ids.dtype == np.int32 and np.array_equal(ids, want_ids)
    out = torch.full(shape, -7, dtype=torch.int16, device="cuda:0")
    got, ids = ctx.regiongrid(shape, gt, polygons=features, values=values, out=out, **kw)
    assert got is out and np.array_equal(out.cpu().numpy(), want) and np.array_equal(ids, want_ids)


@pytest.mark.parametrize("scene", ["hand", "big", "off", "triangle"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_polygons_equal_the_model(ctx, shape, scene):
    for features, values in {"hand": hand_scene, "big": big_scene, "off": off_scene, "triangle": triangle_scene}[scene](shape):
        check(ctx, shape, IDENT, features, values)


def test_hand_cases_on_their_own_rasters(ctx):
    for _, (shape, features, values, want) in sorted(HAND_CASES.items()):
        grid, ids = ctx.regiongrid(shape, IDENT, polygons=features, values=values)
        assert np.array_equal(grid, want) and np.array_equal(ids, M.ids_of(want))


@pytest.mark.parametrize("frame", sorted(UTM))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_polygons_in_a_utm_frame(ctx, shape, frame):
    features, values = random_scene(shape, UTM[frame])
    check(ctx, shape, UTM[frame], features, values)


def test_many_batches(ctx):
    """3 000 unit squares, the workspace bound at two features' bitmaps: a unit square holds one row of centres and its box one or two words,
    so a bound of 2 words lets at most two features into a batch."""
    shape = (70, 300)
    rng = np.random.default_rng(8)
    x0, y0 = rng.uniform(-1, 300, 3000), rng.uniform(-1, 70, 3000)
    features = [[[(x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1)]] for x, y in zip(x0, y0)]
    values = rng.integers(1, 400, 3000).tolist()
    want, want_ids = M.polygons(shape, IDENT, features, values)
    assert want_ids.size > 300
    for ws in (2, 0):
        grid, ids, st = ctx.regiongrid(shape, IDENT, polygons=features, values=values, workspace_words=ws, stats=True)
        assert np.array_equal(grid, want) and np.array_equal(ids, want_ids)
        assert set(st["phases"]) == {"prepare", "cross", "fill", "write"} and st["workspace_bytes"] > 0
        assert st["launches_stencil"] >= (1400 if ws else 1), "the fill kernel runs once per batch"


def test_out_off_the_16_byte_boundary(ctx):
    shape = (33, 65)
    features, values = random_scene(shape, IDENT, seed=9)
    want, _ = M.polygons(shape, IDENT, features, values)
    flat = torch.zeros(33 * 65 + 8, dtype=torch.int16, device="cuda:0")
    out = flat[1:1 + 33 * 65].view(shape)
    assert out.data_ptr() % 16 == 2
    ctx.regiongrid(shape, IDENT, polygons=features, values=values, out=out)
    assert np.array_equal(out.cpu().numpy(), want) and flat[0] == 0 and not flat[1 + 33 * 65:].any()


def test_same_bytes_on_three_runs(ctx):
    shape = (70, 300)
    features, values = random_scene(shape, UTM["north_up_30"])
    runs = [ctx.regiongrid(shape, UTM["north_up_30"], polygons=features, values=values) for _ in range(3)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() == runs[2][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes() == runs[2][1].tobytes()


def test_refusals(ctx):
    sq = [[[(1, 1), (4, 1), (4, 3), (1, 3)]]]
    for v in (0, -1, 32768, 2 ** 40):
        with pytest.raises(T.TdxError, match="feature 1: value .* is outside 1 .. 32767"):
            ctx.regiongrid((5, 6), IDENT, polygons=sq * 2, values=[1, v])
    with pytest.raises(T.TdxError, match="rotated"):
        ctx.regiongrid((5, 6), (0, 1, 0.1, 0, 0, 1), polygons=sq, values=[1])
    with pytest.raises(ValueError):
        ctx.regiongrid((5, 6), IDENT, polygons=sq, values=[1], source=np.zeros((2, 2), np.int32), source_gt=IDENT)
    grid, ids = ctx.regiongrid((5, 6), IDENT, polygons=[], values=[])          # an empty layer: nothing but nodata
    assert not grid.any() and ids.size == 0
    grid, ids = T.regiongrid((5, 6), IDENT, polygons=sq, values=[12])         # the module-level call
    assert np.array_equal(grid, HAND_CASES["square"][3] * 12) and ids.tolist() == [12]


def test_numbers_that_are_not_finite(ctx):
    """A vertex without finite pixel coordinates is refused; finite vertices whose x2 - x1 overflows give crossings at -inf, +inf or NaN, and the
    rule xs < xc holds as written: the model and the device agree."""
    shape = (5, 67)
    for bad in (float("nan"), float("inf"), 1e308):
        ring = [(1.0, 1.0), (bad, 1.0), (4.0, 3.0), (1.0, 3.0)]
        with pytest.raises(T.TdxError, match="feature 0: a vertex without finite pixel coordinates"):
            ctx.regiongrid(shape, (0.0, 1e-3, 0.0, 0.0, 0.0, 1.0), polygons=[[ring]], values=[1])
    with pytest.raises(ValueError, match="finite"):
        M.polygons(shape, IDENT, [[[(1.0, 1.0), (float("nan"), 1.0), (4.0, 3.0)]]], [1])
    huge = [[[(-1.7e308, -1.0), (1.7e308, 2.5), (1.7e308, 7.0), (-1.7e308, 4.0)]], [[(-1.7e308, 0.2), (1.7e308, 4.8), (3.0, 9.0)]]]
    check(ctx, shape, IDENT, huge, [3, 4])


def test_packed_polygons_burn_back_what_the_lists_do(ctx):
    """Polygons.packed(gt) -> PackedPolygons: the same grid as the lists of rings of the same polygons, as the model, and as the watershed grid."""
    import polygonize_model as PM

    for name in ("nested", "blocks_70x300", "checker_64x65", "plain:w_plain"):
        w = GRIDS[name]
        with ctx.polygonize(w, PM.NODATA) as pg:
            packed, ids, feats = pg.packed(GT70), pg.ids.copy(), pg.features()
        assert isinstance(packed, T.PackedPolygons) and len(packed) == ids.size
        shift = 1 - int(ids.min())                  # ids that start at 0 (or below) are burned as id + shift: 0 is the region grid's nodata
        ids = ids + shift
        assert ids.max() <= 32767, name
        lists = [[[(GT70[0] + c * GT70[1], GT70[3] + r * GT70[5]) for c, r in ring] for p in polys for ring in p] for _, _, polys in feats]
        want = np.where(w == PM.NODATA, 0, w + shift).astype(np.int16)
        a, ia = ctx.regiongrid(w.shape, GT70, polygons=packed, values=ids)
        b, ib = ctx.regiongrid(w.shape, GT70, polygons=lists, values=ids)
        assert np.array_equal(a, b) and np.array_equal(a, want) and np.array_equal(ia, ib)
        if w.size <= 70 * 300:
            assert np.array_equal(a, M.polygons(w.shape, GT70, lists, ids)[0])
    with pytest.raises(ValueError, match="one value per feature"):
        ctx.regiongrid(w.shape, GT70, polygons=packed, values=ids[:-1])


# ---- resample and constant
def _source(shape, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(1, 9, shape).astype(np.int32)
    s[rng.random(shape) < 0.1] = -9
    return s


GT70 = (4.1e5, 30.0, 0.0, 4.6e6, 0.0, -30.0)
RESAMPLE = {   # name -> (source shape, source geotransform) against a 70 x 300 raster of 30 m cells from (4.1e5, 4.6e6)
    "finer": ((300, 1000), (4.1e5 - 50, 10.0, 0.0, 4.6e6 + 70, 0.0, -10.0)),
    "coarser": ((30, 100), (4.1e5 - 100, 100.0, 0.0, 4.6e6 + 200, 0.0, -100.0)),
    "offset": ((80, 310), (4.1e5 - 47.3, 30.0, 0.0, 4.6e6 + 33.7, 0.0, -30.0)),
    "smaller": ((20, 50), (4.1e5 + 1000, 30.0, 0.0, 4.6e6 - 500, 0.0, -30.0)),
    "row_flipped": ((80, 310), (4.1e5 - 60, 30.0, 0.0, 4.6e6 - 2250, 0.0, 30.0)),
}


@pytest.mark.parametrize("name", sorted(RESAMPLE))
def test_resample_equals_the_model(ctx, name):
    sshape, sgt = RESAMPLE[name]
    src = _source(sshape, 3)
    want, want_ids, bad = M.resample((70, 300), GT70, src, sgt, -9)
    assert bad == 0 and want.any() and (want == 0).any()        # nodata and cells off the source are in every case
    grid, ids = ctx.regiongrid((70, 300), GT70, source=src, source_gt=sgt, source_nodata=-9)
    assert np.array_equal(grid, want) and np.array_equal(ids, want_ids)
    out = torch.full((70, 300), -7, dtype=torch.int16, device="cuda:0")
    _, ids = ctx.regiongrid((70, 300), GT70, source=torch.from_numpy(src).to("cuda:0"), source_gt=sgt, source_nodata=-9, out=out)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(ids, want_ids)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resample_small_rasters(ctx, shape):
    src = _source((7, 9), 4)
    sgt = (-1.5, shape[1] / 6.0, 0.0, -0.5, 0.0, shape[0] / 5.0)
    want, want_ids, bad = M.resample(shape, IDENT, src, sgt, -9)
    grid, ids = ctx.regiongrid(shape, IDENT, source=src, source_gt=sgt, source_nodata=-9)
    assert bad == 0 and np.array_equal(grid, want) and np.array_equal(ids, want_ids)


def test_resample_refuses_values_outside_int16(ctx):
    sshape, sgt = RESAMPLE["offset"]
    src = _source(sshape, 3)
    src[10:12, 20:25] = 40000
    src[40, 40] = 0
    _, _, bad = M.resample((70, 300), GT70, src, sgt, -9)
    assert bad == 11
    out = torch.full((70, 300), -7, dtype=torch.int16, device="cuda:0")
    with pytest.raises(T.TdxError, match="11 cells take a source value outside 1 .. 32767"):
        ctx.regiongrid((70, 300), GT70, source=torch.from_numpy(src).to("cuda:0"), source_gt=sgt, source_nodata=-9, out=out)
    assert (out == -7).all(), "nothing is written"
    with pytest.raises(T.TdxError, match="11 cells"):
        ctx.regiongrid((70, 300), GT70, source=src, source_gt=sgt, source_nodata=-9)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_constant_mode(ctx, shape):
    grid, ids = ctx.regiongrid(shape, IDENT)
    assert grid.dtype == np.int16 and (grid == 1).all() and ids.tolist() == [1]
    out = torch.zeros(shape, dtype=torch.int16, device="cuda:0")
    ctx.regiongrid(shape, GT70, out=out)
    assert (out == 1).all()


# ---- the round trip: watershed grid -> polygons -> layer file -> region grid
ROUND_TRIP = sorted(k for k, w in GRIDS.items() if ((w >= 1) & (w <= 32767)).any())


def test_the_round_trip_covers_the_named_grids():
    assert {"checker_64x65", "stripes_33x64", "nested", "plain:w_plain", "plain:w_outlets", "plain:w_sw", "holes:w_plain", "geographic:w_outlets"} <= set(ROUND_TRIP)


@pytest.mark.parametrize("name", ROUND_TRIP)
def test_round_trip_gives_the_watershed_grid_back(ctx, name, tmp_path):
    import polygonize_model as PM

    w = GRIDS[name]
    want = np.where((w == PM.NODATA) | (w < 1) | (w > 32767), 0, w).astype(np.int16)
    with ctx.polygonize(w, PM.NODATA) as pg:
        for ext in (".shp", ".geojson"):
            path = str(tmp_path / ("ws" + ext))
            pg.write(path, GT70)
            layer = T.read_polygons(path)
            code = [int(v) for v in layer.fields["gridcode"]]
            keep = [k for k, v in enumerate(code) if 1 <= v <= 32767]        # ids that no region grid can hold are dropped here
            feats = [layer.polygons[k] for k in keep]
            vals = layer.values("gridcode") if len(keep) == len(code) else [code[k] for k in keep]
            grid, ids = ctx.regiongrid(w.shape, GT70, polygons=feats, values=vals)
            assert np.array_equal(grid, want), (ext, np.argwhere(grid != want)[:5])
            assert np.array_equal(ids, M.ids_of(want))


# ---- bin/siregiontool
DEM_SHAPE = (70, 300)


def _tool(args, gpus=None):
    return subprocess.run([os.path.join(BIN, "siregiontool")] + (["--gpus", str(gpus)] if gpus else []) + [str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def tool_dir(tmp_path_factory):
    import regiongrid_files as F

    d = tmp_path_factory.mktemp("siregiontool")
    f = lambda s: str(d / s)  # noqa: E731
    rng = np.random.default_rng(2)
    dem = rng.uniform(100, 200, DEM_SHAPE).astype(np.float32)
    dem[3:6, 10:20] = -9999.0
    T.write_raster(f("dem.tif"), dem, -9999.0, geotransform=GT70)
    features, values = random_scene(DEM_SHAPE, GT70, seed=21)
    values = [v * 100 for v in values]
    F.write_layer(f("regions.shp"), 5, features, field="REGION", texts=[str(v) for v in values])
    sshape, sgt = RESAMPLE["offset"]
    src = _source(sshape, 6)
    T.write_raster(f("regions.tif"), src, -9, geotransform=sgt)
    return f, (features, values), (src, sgt)


def _check_outputs(f, parreg, att, want, want_ids, texts=("2.708", "2.708", "0.0", "0.25", "30.0", "45.0", "2000.0")):
    import peuker_model as PM

    grid, info = T.read_raster(f(parreg), np.int16)
    assert np.array_equal(grid, want) and info["nodata"] == 0 and info["has_nodata"] and info["geotransform"] == T.raster_info(f("dem.tif"))["geotransform"]
    assert PM.tiff_sample_type(f(parreg)) == (16, 2)                        # 16 bits, signed integers
    assert open(f(att)).read() == M.table_text(want_ids, texts)
    assert T.read_calpar(f(att))["id"].tolist() == want_ids.tolist()


@pytest.mark.parametrize("gpus", [None, 2])
def test_tool_three_modes(tool_dir, gpus):
    f, (features, values), (src, sgt) = tool_dir
    if gpus and torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    tag = f"_{gpus or 1}"
    p = _tool(["--dem", f("dem.tif"), "--parreg", f("one" + tag + ".tif"), "--att", f("one" + tag + ".csv")], gpus)
    assert p.returncode == 0 and p.stdout.endswith("Region computation successful.\n") and f"Processes: {gpus or 1}\n" in p.stdout, p.stdout + p.stderr
    _check_outputs(f, "one" + tag + ".tif", "one" + tag + ".csv", *M.constant(DEM_SHAPE))
    p = _tool(["--dem", f("dem.tif"), "--shp", f("regions.shp"), "--shp-att-name", "REGION", "--parreg", f("shp" + tag + ".tif"), "--att", f("shp" + tag + ".csv"),
               "--att-tmin", "1.5", "--att-cmax=0.30", "--att-soildens", "1.9e3"], gpus)
    assert p.returncode == 0 and p.stdout.endswith("Region computation successful.\n"), p.stdout + p.stderr
    want, want_ids = M.polygons(DEM_SHAPE, GT70, features, values)
    assert want_ids.size >= 3
    _check_outputs(f, "shp" + tag + ".tif", "shp" + tag + ".csv", want, want_ids, ("1.5", "2.708", "0.0", "0.30", "30.0", "45.0", "1.9e3"))
    p = _tool(["--dem", f("dem.tif"), "--parreg-in", f("regions.tif"), "--parreg", f("src" + tag + ".tif"), "--att", f("src" + tag + ".csv")], gpus)
    assert p.returncode == 0 and p.stdout.endswith("Region computation successful.\n"), p.stdout + p.stderr
    want, want_ids, bad = M.resample(DEM_SHAPE, GT70, src, sgt, -9)
    assert bad == 0
    _check_outputs(f, "src" + tag + ".tif", "src" + tag + ".csv", want, want_ids)


def test_tool_refusals(tool_dir):
    f = tool_dir[0]
    before = sorted(os.listdir(os.path.dirname(f("x"))))
    p = _tool(["--dem", f("dem.tif"), "--shp", f("regions.gpkg"), "--parreg", f("no.tif"), "--att", f("no.csv")])
    assert p.returncode == 1 and p.stdout.startswith("Region computation failed.\nsiregiontool: unsupported input"), p.stdout + p.stderr
    p = _tool(["--dem", f("dem.tif"), "--shp", f("regions.shp"), "--parreg-in", f("regions.tif"), "--parreg", f("no.tif"), "--att", f("no.csv")])
    assert p.returncode == 1 and p.stdout.startswith("Region computation failed.\n") and "both given" in p.stdout
    p = _tool(["--dem", f("dem.tif"), "--shp", f("regions.shp"), "--parreg", f("no.tif"), "--att", f("no.csv")])             # the default field ID is not in the layer
    assert p.returncode == 1 and p.stdout.endswith("Region computation failed.\nsiregiontool: the polygon layer has no field ID\n"), p.stdout
    p = _tool(["--dem", f("dem.tif"), "--shp", f("regions.shp"), "--shp-att-name", "FID", "--parreg", f("no.tif"), "--att", f("no.csv")])
    assert p.returncode == 1 and "FID is the record number" in p.stdout
    assert _tool(["--dem", f("dem.tif")]).stdout.startswith("Usage: ")
    assert sorted(os.listdir(os.path.dirname(f("x")))) == before


def test_sinmapsi_runs_on_the_tools_files(ctx, tool_dir, tmp_path):
    """bin/sinmapsi on the region grid and table of bin/siregiontool gives what Context.sinmapsi gives on the model's grid and the table read back."""
    import sinmap_model as SM

    f, (features, values), _ = tool_dir
    p = _tool(["--dem", f("dem.tif"), "--shp", f("regions.shp"), "--shp-att-name", "REGION", "--parreg", f("cal.tif"), "--att", f("calpar.csv")])
    assert p.returncode == 0, p.stdout + p.stderr
    rng = np.random.default_rng(4)
    slp = rng.uniform(0.01, 1.2, DEM_SHAPE).astype(np.float32)
    sca = rng.uniform(30.0, 5000.0, DEM_SHAPE).astype(np.float32)
    T.write_raster(f("slp.tif"), slp, -1.0, geotransform=GT70)
    T.write_raster(f("sca.tif"), sca, -1.0, geotransform=GT70)
    par = [repr(SM.RMINTER), repr(SM.RMAXTER), repr(SM.G), repr(SM.RHOW)]
    q = subprocess.run([os.path.join(BIN, "sinmapsi"), "-slp", f("slp.tif"), "-sca", f("sca.tif"), "-calpar", f("calpar.csv"), "-cal", f("cal.tif"), "-si", f("si.tif"),
                        "-sat", f("sat.tif"), "-par", *par], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0, q.stdout + q.stderr
    cal, _ = M.polygons(DEM_SHAPE, GT70, features, values)
    si, sat = ctx.sinmapsi(slp, sca, cal, T.read_calpar(f("calpar.csv")), float(np.float32(SM.RMINTER)), float(np.float32(SM.RMAXTER)), SM.G, float(np.float32(SM.RHOW)),
                           slp_nodata=-1.0, cal_nodata=0)
    got_si, got_sat = T.read_raster(f("si.tif"))[0], T.read_raster(f("sat.tif"))[0]
    assert np.array_equal(got_si.view(np.uint32), si.view(np.uint32)) and np.array_equal(got_sat.view(np.uint32), sat.view(np.uint32))
    assert np.unique(cal[cal != 0]).size >= 3 and np.isfinite(si[cal != 0]).all()        # several regions took part
