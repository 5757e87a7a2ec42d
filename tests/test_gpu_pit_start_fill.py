"""PitRemove's coarse-to-fine start with ONE seed pass: pit_seed_kernel<3> writes the first coarse level and the unprolonged seed surface W0, and the fine
level's first run (PitStartOp, taudem_amd/csrc/pitremove.hip) reads a cell that still holds FLT_MAX as the relaxed coarse value of its 8 x 8 block and stores
every cell it filled.  Every result is compared bit for bit with the restatement (src/flood.cpp:243-479), by default and under TDX_PIT_SEED=two (the two
streaming passes).  The coarse path needs 2^18 cells in all strips: the rasters are just above that."""
import numpy as np
import pytest

import pathological
from conftest import bits_equal, describe_diff

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234663852886e38)
NODATA = -9999.0
SEED_MODES = [None, "two"]
SCHEDULES = [{}, {"TDX_PIT_VCYCLE_AFTER": "0"}, {"TDX_PIT_VCYCLE_AFTER": "1", "TDX_PIT_VCYCLE_MIN": "0"}, {"TDX_ACT_FILTER_OFF": "1"}]


def _seeded(oracle, shape, seed):
    return oracle.synth_dem(shape, seed)


def _nodata_raster(oracle):
    """Holes that cover whole 8 x 8 blocks, holes that cut blocks, holes along a tile rim (columns 63 / 64, rows 127 / 128)."""
    z = oracle.synth_dem((600, 520), 21).copy()
    z[64:96, 200:232] = NODATA      # sixteen whole blocks
    z[400:408, 8:16] = NODATA       # one whole block
    z[131:150, 301:333] = NODATA    # cuts blocks on all four sides
    z[300:420, 60:64] = NODATA      # ends on column 63
    z[200:290, 64:67] = NODATA      # starts on column 64
    z[124:128, 100:300] = NODATA    # ends on row 127
    z[128:131, 320:500] = NODATA    # starts on row 128
    z[127:129, 40:50] = NODATA      # across the rim
    return z


def _seed_mask(shape):
    rng = np.random.default_rng(5)
    m = np.zeros(shape, np.int16)
    ys = rng.integers(40, shape[0] - 40, 300)
    xs = rng.integers(40, shape[1] - 40, 300)
    m[ys, xs] = 1
    return m


def _plateau():
    """A 200 x 200 plateau at the height of its outlet inside higher ground: W* = Z = Wc on it, no sweep ever lowers one of its cells."""
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:560, 0:520]
    z = (100.0 + 0.01 * x + 0.02 * y + rng.random((560, 520))).astype(np.float32)
    z[200:400, 150:350] = np.float32(50.0)
    z[300, 0:150] = np.float32(50.0)   # the outlet: a level channel to the west edge
    return z


def _basin_spill_is_block_maximum():
    """A basin behind a wall one block thick whose only gap is one aligned block: floor 55, one column of it 60 - the spill, and the largest elevation of its block."""
    rng = np.random.default_rng(9)
    y, x = np.mgrid[0:540, 0:520]
    z = (30.0 - 0.01 * x + rng.random((540, 520)) * 0.5).astype(np.float32)
    z[96:304, 96:304] = np.float32(80.0)
    z[104:296, 104:296] = (10.0 + rng.random((192, 192))).astype(np.float32)
    z[200:208, 96:104] = np.float32(55.0)
    z[200:208, 100] = np.float32(60.0)
    return z


def _lake_across_cuts(oracle):
    """(700, 900) with a closed basin over rows 120 ... 480: across the cuts of three strips (233, 466) and of five (140, 280, 420)."""
    z = oracle.synth_dem((700, 900), 4).copy()
    rng = np.random.default_rng(2)
    z[120:480, 300:500] = (z.min() - 10.0 + rng.random((360, 200))).astype(np.float32)
    return z


_CACHE = {}


def _case(oracle, name):
    """(dem, mask, reference), computed once per module run and never written to."""
    if name not in _CACHE:
        mask = None
        if name == "seeded_523x517":
            dem = _seeded(oracle, (523, 517), 3)
        elif name == "seeded_700x900":
            dem = _seeded(oracle, (700, 900), 4)
        elif name == "nodata":
            dem = _nodata_raster(oracle)
        elif name == "nodata_mask":
            dem = _nodata_raster(oracle)
            mask = _seed_mask(dem.shape)
        elif name == "constant":
            dem = pathological.plane(523, 517)
        elif name == "plateau":
            dem = _plateau()
        elif name == "basin":
            dem = _basin_spill_is_block_maximum()
        elif name == "checkerboard":
            dem = pathological.checkerboard_pits(640, 640)
        elif name == "spiral":
            dem = pathological.spiral(640)
        elif name == "lake_700x900":
            dem = _lake_across_cuts(oracle)
        else:
            raise KeyError(name)
        assert dem.size >= 1 << 18
        ref = oracle.pitremove(dem, NODATA, mask=mask)
        for a in (dem, ref) + ((mask,) if mask is not None else ()):
            a.setflags(write=False)
        _CACHE[name] = (dem, mask, ref)
    return _CACHE[name]


def _setenv(monkeypatch, seed_mode, env):
    for k in ("TDX_PIT_SEED", "TDX_PIT_VCYCLE_AFTER", "TDX_PIT_VCYCLE_MIN", "TDX_ACT_FILTER_OFF", "TDX_PIT_NO_COARSE"):
        monkeypatch.delenv(k, raising=False)
    if seed_mode:
        monkeypatch.setenv("TDX_PIT_SEED", seed_mode)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run(ctx, dem, mask, seed_mode, coarse=True, **kw):
    fel, st = ctx.pitremove(np.array(dem), NODATA, mask=None if mask is None else np.array(mask), stats=True, **kw)   # (copies: the shared rasters are read-only)
    if coarse:   # the path under test was taken: one streaming pass, or today's two
        assert st["launches_stencil"] == (2 if seed_mode == "two" else 1), st
    return fel


def _no_fltmax(fel, dem):
    valid = dem != np.float32(NODATA)
    return not np.any(fel[valid] == FLT_MAX)


@pytest.mark.parametrize("seed_mode", SEED_MODES)
@pytest.mark.parametrize("env", SCHEDULES, ids=["default", "no_vcycle", "vcycle_after_1", "act_filter_off"])
@pytest.mark.parametrize("name", ["seeded_523x517", "seeded_700x900"])
def test_seeded_dems(ctx, oracle, monkeypatch, name, env, seed_mode):
    dem, mask, ref = _case(oracle, name)
    _setenv(monkeypatch, seed_mode, env)
    fel = _run(ctx, dem, mask, seed_mode)
    assert bits_equal(fel, ref), describe_diff(fel, ref, f"fel {name} {env} seed={seed_mode}")


@pytest.mark.parametrize("seed_mode", SEED_MODES)
def test_out_prefilled_with_nan(ctx, oracle, monkeypatch, seed_mode):
    dem, mask, ref = _case(oracle, "seeded_523x517")
    _setenv(monkeypatch, seed_mode, {})
    out = np.full(dem.shape, np.nan, np.float32)
    fel = _run(ctx, dem, mask, seed_mode, out=out)
    assert fel is out
    assert bits_equal(out, ref), describe_diff(out, ref, f"fel into out= seed={seed_mode}")


@pytest.mark.parametrize("seed_mode", SEED_MODES)
@pytest.mark.parametrize("kind", ["fourway", "no_coarse"])
def test_untouched_paths(ctx, oracle, monkeypatch, kind, seed_mode):
    """The four-neighbour fill and TDX_PIT_NO_COARSE=1 take pit_seed_kernel<0> and the plain operator whatever the switch says."""
    dem, _, ref8 = _case(oracle, "seeded_523x517")
    _setenv(monkeypatch, seed_mode, {"TDX_PIT_NO_COARSE": "1"} if kind == "no_coarse" else {})
    fel, st = ctx.pitremove(np.array(dem), NODATA, fourway=kind == "fourway", stats=True)
    assert st["launches_stencil"] == 1
    if kind == "fourway":
        if "fourway" not in _CACHE:
            _CACHE["fourway"] = oracle.pitremove(dem, NODATA, fourway=True)
        ref = _CACHE["fourway"]
    else:
        ref = ref8
    assert bits_equal(fel, ref), describe_diff(fel, ref, f"fel {kind} seed={seed_mode}")


@pytest.mark.parametrize("seed_mode", SEED_MODES)
@pytest.mark.parametrize("env", SCHEDULES, ids=["default", "no_vcycle", "vcycle_after_1", "act_filter_off"])
def test_nodata_holes(ctx, oracle, monkeypatch, env, seed_mode):
    dem, mask, ref = _case(oracle, "nodata")
    _setenv(monkeypatch, seed_mode, env)
    fel = _run(ctx, dem, mask, seed_mode)
    assert bits_equal(fel, ref), describe_diff(fel, ref, f"fel nodata {env} seed={seed_mode}")
    assert _no_fltmax(fel, dem)


@pytest.mark.parametrize("seed_mode", SEED_MODES)
def test_nodata_holes_with_seed_mask(ctx, oracle, monkeypatch, seed_mode):
    dem, mask, ref = _case(oracle, "nodata_mask")
    assert 250 <= int(mask.sum()) <= 300
    _setenv(monkeypatch, seed_mode, {})
    fel = _run(ctx, dem, mask, seed_mode)
    assert bits_equal(fel, ref), describe_diff(fel, ref, f"fel nodata + mask seed={seed_mode}")
    assert _no_fltmax(fel, dem)


@pytest.mark.parametrize("seed_mode", SEED_MODES)
@pytest.mark.parametrize("name", ["constant", "plateau", "basin", "checkerboard", "spiral"])
def test_cells_the_sweeps_never_move(ctx, oracle, monkeypatch, name, seed_mode):
    """A filled cell that no sweep lowers is still stored: nothing valid is left at FLT_MAX."""
    dem, mask, ref = _case(oracle, name)
    _setenv(monkeypatch, seed_mode, {})
    fel = _run(ctx, dem, mask, seed_mode)
    assert _no_fltmax(fel, dem), f"{name}: {int(np.sum(fel == FLT_MAX))} cells left at FLT_MAX"
    assert bits_equal(fel, ref), describe_diff(fel, ref, f"fel {name} seed={seed_mode}")
    if name == "plateau":   # (what the raster was built for, stated on the reference)
        assert np.all(ref[200:400, 150:350] == np.float32(50.0))
    if name == "basin":
        assert np.all(ref[104:296, 104:296] == np.float32(60.0)) and dem[200:208, 96:104].max() == np.float32(60.0)


def _in_strips(dem, size):
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows

    ny, nx = dem.shape
    parts = partition_rows(ny, size)
    assert all((y1 - y0) % 8 for y0, y1 in parts), "a rank's last coarse row must be a cut block row"
    dem_t = torch.from_numpy(np.array(dem))
    with StripGroup(size, nx) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            pipe = StripPipeline(c, comm, nx, y1 - y0)
            z = pipe.empty(torch.float32)
            z[1:y1 - y0 + 1].copy_(dem_t[y0:y1])
            fel, st = pipe.pitremove(z, NODATA)
            torch.cuda.synchronize()
            return fel[1:y1 - y0 + 1].cpu().numpy(), st["launches_stencil"]
        res = grp.run(rank_main)
    return np.concatenate([r[0] for r in res]), [r[1] for r in res]


@pytest.mark.parametrize("seed_mode", SEED_MODES)
@pytest.mark.parametrize("name,size", [("seeded_523x517", 2), ("seeded_523x517", 3), ("lake_700x900", 3), ("lake_700x900", 5)])
def test_strips(ctx, oracle, monkeypatch, name, size, seed_mode):
    dem, mask, ref = _case(oracle, name)
    _setenv(monkeypatch, seed_mode, {})
    key = ("one_strip", name)
    if key not in _CACHE:   # the one-strip result of the default path
        _setenv(monkeypatch, None, {})
        _CACHE[key] = _run(ctx, dem, mask, None)
        _CACHE[key].setflags(write=False)
        _setenv(monkeypatch, seed_mode, {})
    one = _CACHE[key]
    fel, stencils = _in_strips(dem, size)
    assert stencils == [2 if seed_mode == "two" else 1] * size
    assert bits_equal(fel, one), describe_diff(fel, one, f"fel {name} in {size} strips against one strip, seed={seed_mode}")
    assert bits_equal(fel, ref), describe_diff(fel, ref, f"fel {name} in {size} strips, seed={seed_mode}")
    assert _no_fltmax(fel, dem)


def test_strips_without_coarse_correction(ctx, oracle, monkeypatch):
    """TDX_PIT_VCYCLE_AFTER=0 in strips: the start operator runs as pit_relax_level's first run, and the halo rows still hold W0 until the first exchange."""
    dem, mask, ref = _case(oracle, "lake_700x900")
    _setenv(monkeypatch, None, {"TDX_PIT_VCYCLE_AFTER": "0"})
    fel, stencils = _in_strips(dem, 3)
    assert stencils == [1, 1, 1]
    assert bits_equal(fel, ref), describe_diff(fel, ref, "fel lake in 3 strips, no coarse correction")


def test_six_calls_on_one_context(oracle, monkeypatch):
    """Scratch reuse: two sizes and the two seed paths in turn on one context."""
    import taudem_amd

    a, b = _case(oracle, "seeded_523x517"), _case(oracle, "seeded_700x900")
    with taudem_amd.Context(0) as c:
        for i, ((dem, mask, ref), seed_mode) in enumerate([(a, None), (b, "two"), (a, "two"), (b, None), (a, None), (b, None)]):
            _setenv(monkeypatch, seed_mode, {})
            fel = _run(c, dem, mask, seed_mode)
            assert bits_equal(fel, ref), describe_diff(fel, ref, f"call {i} shape={dem.shape} seed={seed_mode}")
