"""The region grid on row strips (StripPipeline.regiongrid): cuts at 2, at 3 and with every row a strip of its own.  The owned rows equal the
one-device result, the halo rows - filled with a poison value beforehand - are unwritten, and the union of the strips' ids is the raster's.  Nothing is
exchanged: every strip is computed on its own with the raster's geotransform, its first row and the raster's row count."""
import numpy as np
import pytest
import torch

import regiongrid_model as M
from taudem_amd.distributed import StripPipeline
from test_gpu_polygonize import cuts_of
from test_gpu_regiongrid import GT70, IDENT, RESAMPLE, UTM, _source, big_scene, random_scene, triangle_scene

pytestmark = pytest.mark.gpu

POISON = -12345


def run_strips(ctx, shape, cuts, gt, **kw):
    ny, nx = shape
    bounds = [0] + list(cuts) + [ny]
    rows, ids = [], set()
    for y0, y1 in zip(bounds[:-1], bounds[1:]):
        out = torch.full((y1 - y0 + 2, nx), POISON, dtype=torch.int16, device="cuda:0")
        got, strip_ids, st = StripPipeline(ctx, None, nx, y1 - y0).regiongrid(gt, y0, ny, out=out, **kw)
        assert got is out and "ms_total" in st
        a = out.cpu().numpy()
        assert (a[0] == POISON).all() and (a[-1] == POISON).all(), "the halo rows are not written"
        assert np.array_equal(strip_ids, M.ids_of(a[1:-1])), "a strip's ids are those of its owned rows"
        rows.append(a[1:-1])
        ids |= set(strip_ids.tolist())
    return np.concatenate(rows), np.array(sorted(ids), np.int32)


SCENES = {
    "random_70x300": ((70, 300), lambda s: random_scene(s, UTM["north_up_30"]), UTM["north_up_30"]),
    "random_33x65_south_up": ((33, 65), lambda s: random_scene(s, UTM["south_up_10x25"]), UTM["south_up_10x25"]),
    "around_and_dent_5x67": ((5, 67), lambda s: big_scene(s)[2], IDENT),
    "triangle_41x1": ((41, 1), lambda s: triangle_scene(s)[0], IDENT),
    "triangle_70x300": ((70, 300), lambda s: triangle_scene(s)[0], IDENT),
}


@pytest.mark.parametrize("how", [2, 3, "rows"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_polygon_strips_equal_one_device(ctx, name, how):
    shape, scene, gt = SCENES[name]
    features, values = scene(shape)
    want, want_ids = M.polygons(shape, gt, features, values)
    one, one_ids = ctx.regiongrid(shape, gt, polygons=features, values=values)
    assert np.array_equal(one, want)
    grid, ids = run_strips(ctx, shape, cuts_of(shape[0], how), gt, polygons=features, values=values)
    assert np.array_equal(grid, one) and np.array_equal(ids, one_ids) and np.array_equal(ids, want_ids)


@pytest.mark.parametrize("how", [2, 3, "rows"])
@pytest.mark.parametrize("name", ["finer", "offset", "row_flipped"])
def test_resample_strips_equal_one_device(ctx, name, how):
    sshape, sgt = RESAMPLE[name]
    src = _source(sshape, 3)
    want, want_ids, _ = M.resample((70, 300), GT70, src, sgt, -9)
    d_src = torch.from_numpy(src).to("cuda:0")
    grid, ids = run_strips(ctx, (70, 300), cuts_of(70, how), GT70, source=d_src, source_gt=sgt, source_nodata=-9)
    assert np.array_equal(grid, want) and np.array_equal(ids, want_ids)


@pytest.mark.parametrize("how", [2, "rows"])
def test_constant_strips(ctx, how):
    grid, ids = run_strips(ctx, (41, 37), cuts_of(41, how), IDENT)
    assert (grid == 1).all() and ids.tolist() == [1]


def test_a_strip_refuses_what_the_raster_refuses(ctx):
    import taudem_amd as T

    sshape, sgt = RESAMPLE["offset"]
    src = _source(sshape, 3)
    src[40, 40] = 40000            # taken by cells of the lower rows only
    want_bad = M.resample((70, 300), GT70, src, sgt, -9)[2]
    assert want_bad == 1
    d_src = torch.from_numpy(src).to("cuda:0")
    out = torch.full((37, 300), POISON, dtype=torch.int16, device="cuda:0")
    with pytest.raises(T.TdxError, match="1 cells take a source value outside"):
        StripPipeline(ctx, None, 300, 35).regiongrid(GT70, 35, 70, source=d_src, source_gt=sgt, source_nodata=-9, out=out)
    assert (out == POISON).all()
    StripPipeline(ctx, None, 300, 35).regiongrid(GT70, 0, 70, source=d_src, source_gt=sgt, source_nodata=-9, out=out)   # the upper half does not take it
    assert (out[1:-1] != POISON).all()
