"""Per-row cell sizes (geographic rasters) through every table that carries them: the D8 distance table fact[m*9+k] (slopes and flat
resolution), D-infinity's row geometry (slope stencil, flat directions), the accumulations' per-row proportions and cell areas (the donor's
row and the cell's own), the limited accumulations' tile-local row copies, GridNet's distances - at shapes of one tile, many tile rows
and many tile columns, in every flat form and, for the large sweeps, on both tile geometries.  The row sizes come from tests/cellsizes.py:
the product's own reader on a geographic raster (mid-latitude fine cells; a coarse band from 70 N to 40 N) and `wild` rows whose dx / dy
jumps between 0.2 and 5 from one row to the next.  Everything is compared with the restatement (the 1-rank reference), bit for bit.

The halo geometry of a strip: a strip's first and last rows read donors in the halo rows, and the geometry of a
halo row is that of the neighbouring GLOBAL row (rows_of in tool_strips.hpp, taudem_amd.distributed.strip_rows) - what the reference
computes on one rank.  On several ranks the reference's getdxdyc() leaves a halo row's sizes at whatever the previous call read
(src/linearpart.h:531-534), so its rasters depend on the rank count: on a 300 x 200 geographic raster (70 N -> 40 N, 0.1 degree cells)
AreaDinf -nc differs between 1 and 3 ranks in 3 229 cells (DinfRevAccum: 3 218), all of them downstream of cells in the strips' edge
rows.  The 1-rank reference is the only well-defined target; these tests and the strip tests hold the product to it."""
import numpy as np
import pytest

from cellsizes import KINDS, rows
from conftest import bits_equal, describe_diff

pytestmark = pytest.mark.gpu
ANG_ND = -3.402823466e38
SHAPES = [(1000, 777), (4100, 96), (96, 4100), (257, 301), (65, 64), (64, 129)]
CASES = [(shape, kind) for shape in SHAPES for kind in KINDS]
IDS = [f"{s[0]}x{s[1]}-{k}" for s, k in CASES]


def same(a, b, name):
    assert bits_equal(a, b), describe_diff(a, b, name)


def _fel(oracle, shape, seed, quantum=None):
    dem = oracle.synth_dem(shape, seed)
    if quantum is not None:   # terraces: flats that span many rows and tile rows
        dem = (np.floor(dem / np.float32(quantum)) * np.float32(quantum)).astype(np.float32)
    return oracle.pitremove(dem, -9999.0)


def _outlets(a, rng, count=6):
    """`count` cells among the 400 of largest area, plus the raster's first and last cell."""
    pick = rng.choice(np.argsort(a, axis=None)[-400:], size=min(count, a.size), replace=False)
    oy, ox = np.unravel_index(pick, a.shape)
    ny, nx = a.shape
    return np.r_[ox, 0, nx - 1].astype(np.int32), np.r_[oy, 0, ny - 1].astype(np.int32)


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_d8flowdir_and_gridnet(shape, kind, ctx, oracle):
    dx, dy = rows(kind, shape[0], seed=shape[1])
    fel = _fel(oracle, shape, 3 + shape[1])
    p_o, sd8_o, st_o = oracle.d8flowdir(fel, -3.0e38, dx, dy)
    p, sd8, st = ctx.d8flowdir(fel, -3.0e38, dx, dy, stats=True)
    same(sd8, sd8_o, "sd8")
    same(p, p_o, "p")
    assert (st["flats_initial"], st["flat_iterations"], st["flats_left"]) == (st_o["flats_initial"], st_o["flat_iterations"], st_o["flats_left"]), (st, st_o)
    rng = np.random.default_rng(shape[0])
    a = oracle.aread8(p_o, -32768, contcheck=False)
    outl = _outlets(a, rng)
    mask = np.where(a < 0, -3, a).astype(np.int32)
    for kw, what in ((dict(), "plain"), (dict(mask=mask, thresh=3), "mask, thresh 3"), (dict(outlets=outl), "outlets")):
        for x, y, nm in zip(ctx.gridnet(p_o, -32768, dx, dy, **kw), oracle.gridnet(p_o, -32768, dx, dy, **kw), ("plen", "tlen", "gord")):
            same(np.asarray(x), np.asarray(y), f"gridnet {nm}, {what}")


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_dinfflowdir(shape, kind, ctx, oracle):
    dx, dy = rows(kind, shape[0], seed=shape[1])
    fel = _fel(oracle, shape, 3 + shape[1])
    ang_o, slp_o, st_o = oracle.dinfflowdir(fel, -3.0e38, dx, dy)
    ang, slp, st = ctx.dinfflowdir(fel, -3.0e38, dx, dy, stats=True)
    same(slp, slp_o, "slp")
    same(ang, ang_o, "ang")
    assert (st["flats_initial"], st["flats_left"]) == (st_o["flats_initial"], st_o["flats_left"]), (st, st_o)


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_dinf_accumulations_from_the_oracles_angles(shape, kind, ctx, oracle, monkeypatch):
    """Every accumulation tool on the RESTATEMENT's angles (both sides sweep the same graph), the default tile sweeps and the pull walk."""
    dx, dy = rows(kind, shape[0], seed=shape[1])
    fel = _fel(oracle, shape, 3 + shape[1])
    ang, _, _ = oracle.dinfflowdir(fel, -3.0e38, dx, dy)
    rng = np.random.default_rng(7 + shape[1])
    w = (rng.random(shape, dtype=np.float32) * 3.0 + np.float32(0.25)).astype(np.float32)
    dm = (0.9 + 0.1 * rng.random(shape, dtype=np.float32)).astype(np.float32)
    outl = _outlets(oracle.areadinf(ang, ANG_ND, dx, dy, contcheck=False), rng)
    for walk in (False, True):
        if walk:
            monkeypatch.setenv("TDX_DINF_WALK", "1")
        how = " (walk)" if walk else ""
        for kw, what in ((dict(contcheck=True), "contcheck"), (dict(contcheck=False), "-nc"), (dict(weights=w, contcheck=False), "weights -nc"),
                         (dict(contcheck=True, outlets=outl), "outlets"), (dict(weights=w, contcheck=False, outlets=outl), "weights, outlets -nc")):
            same(ctx.areadinf(ang, ANG_ND, dx, dy, **kw), oracle.areadinf(ang, ANG_ND, dx, dy, **kw), f"sca{how}, {what}")
        for kw, what in ((dict(), "contcheck"), (dict(weights=w, contcheck=False), "weights -nc"), (dict(weights=w, contcheck=True, outlets=outl), "weights, outlets")):
            same(ctx.dinfdecayaccum(ang, dm, ANG_ND, -9999.0, dx, dy, **kw), oracle.dinfdecayaccum(ang, dm, ANG_ND, -9999.0, dx, dy, **kw), f"dsca{how}, {what}")
        monkeypatch.delenv("TDX_DINF_WALK", raising=False)
    dg = (rng.random(shape) < 0.02).astype(np.int32)
    same(ctx.dinfupdependence(ang, dg, dx=dx, dy=dy), oracle.dinfupdependence(ang, dg, dx=dx, dy=dy), "dep")
    for x, y, nm in zip(ctx.dinfrevaccum(ang, w, dx=dx, dy=dy), oracle.dinfrevaccum(ang, w, dx=dx, dy=dy), ("racc", "dmax")):
        same(x, y, nm)
    q = (0.5 + rng.random(shape, dtype=np.float32)).astype(np.float32)
    dg16 = dg.astype(np.int16)
    tc = (rng.random(shape, dtype=np.float32) * 50).astype(np.float32)
    for kw, what in ((dict(), "contcheck"), (dict(contcheck=False, outlets=outl), "outlets -nc")):
        same(ctx.dinfconclimaccum(ang, dm, dg16, q, csol=1.5, dx=dx, dy=dy, **kw), oracle.dinfconclimaccum(ang, dm, dg16, q, csol=1.5, dx=dx, dy=dy, **kw),
             f"ctpt, {what}")
        for c_in in (None, dm):
            for x, y, nm in zip(ctx.dinftranslimaccum(ang, w, tc, cs=c_in, dx=dx, dy=dy, **kw), oracle.dinftranslimaccum(ang, w, tc, cs=c_in, dx=dx, dy=dy, **kw),
                                ("tla", "tdep", "ctpt")):
                if y is not None:
                    same(x, y, f"{nm}{' (cs)' if c_in is not None else ''}, {what}")


FLAT_FORMS = {"stream+blocks": {}, "stream": {"TDX_FLATS_MACRO": "0"}, "list": {"TDX_FLATS_LIST": "1"}, "int32": {"TDX_LEVELS_INT32": "1"}}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", list(FLAT_FORMS))
def test_flat_resolution_under_per_row_distances(form, kind, ctx, oracle, monkeypatch):
    """Elevations on 3 m terraces: flats of thousands of cells across many rows and tile rows, a dense first queue (more than 1/16 of the raster).
    Their directions follow the per-row distance table (D8: fact[m*9+k], D-infinity: the row geometry); D8FlowDir and DinfFlowDir in every flat form
    against the restatement, and in three strips (halo rows from taudem_amd.distributed.strip_rows) against the one-strip run."""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline, partition_rows, strip_rows

    shape = (700, 600)
    ny, nx = shape
    dx, dy = rows(kind, ny, seed=5)
    fel = _fel(oracle, shape, 21, quantum=3.0)
    p_o, sd8_o, st_o = oracle.d8flowdir(fel, -3.0e38, dx, dy)
    ang_o, slp_o, sti_o = oracle.dinfflowdir(fel, -3.0e38, dx, dy)
    assert st_o["flats_initial"] > ny * nx // 16 and st_o["flat_iterations"] >= 2
    for k, v in FLAT_FORMS[form].items():
        monkeypatch.setenv(k, v)
    p, sd8, st = ctx.d8flowdir(fel, -3.0e38, dx, dy, stats=True)
    same(sd8, sd8_o, f"sd8, {form}")
    same(p, p_o, f"p, {form}")
    assert (st["flats_initial"], st["flat_iterations"], st["flats_left"]) == (st_o["flats_initial"], st_o["flat_iterations"], st_o["flats_left"]), (st, st_o)
    ang, slp, sti = ctx.dinfflowdir(fel, -3.0e38, dx, dy, stats=True)
    same(slp, slp_o, f"slp, {form}")
    same(ang, ang_o, f"ang, {form}")
    assert (sti["flats_initial"], sti["flats_left"]) == (sti_o["flats_initial"], sti_o["flats_left"])
    parts = partition_rows(ny, 3)
    fel_t = torch.from_numpy(fel)
    with StripGroup(3, nx) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            pipe = StripPipeline(c, comm, nx, y1 - y0)
            f = pipe.empty(torch.float32)
            f[1:y1 - y0 + 1].copy_(fel_t[y0:y1])
            sdx, sdy = strip_rows(dx, y0, y1), strip_rows(dy, y0, y1)
            pp, ss, _ = pipe.d8flowdir(f, -3.0e38, sdx, sdy)
            aa, sl, _ = pipe.dinfflowdir(f, -3.0e38, sdx, sdy)
            torch.cuda.synchronize()
            return [t[1:y1 - y0 + 1].cpu().numpy() for t in (pp, ss, aa, sl)]
        res = grp.run(rank_main)
    for i, (ref, nm) in enumerate(((p_o, "p"), (sd8_o, "sd8"), (ang_o, "ang"), (slp_o, "slp"))):
        same(np.concatenate([r[i] for r in res]), ref, f"{nm} in three strips, {form}")


@pytest.mark.slow
def test_every_sweep_tool_on_both_tile_geometries_with_wild_rows(ctx, oracle, monkeypatch):
    """tests/test_flowalg.py::test_every_sweep_tool_on_both_tile_geometries with `wild` per-row sizes: 3100 x 2900 (the generic sweep starts on 32 x 32
    tiles and hands over to 64 x 64 ones), every sweep re-checked by TDX_SWEEP_VERIFY=1, and AreaDinf / DinfDecayAccum once more as the pull walk.
    The directions are the restatement's, so that both sides sweep the same graph."""
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    rng = np.random.default_rng(2025)
    shape = (3100, 2900)
    dx, dy = rows("wild", shape[0], seed=11)
    dem = oracle.synth_dem(shape, 61)
    dem[1200:1260, 800:1100] = -9999.0
    fel = oracle.pitremove(dem, -9999.0)
    p, _, _ = oracle.d8flowdir(fel, -3.0e38, dx, dy)
    ang, _, _ = oracle.dinfflowdir(fel, -3.0e38, dx, dy)
    w = (rng.random(shape, dtype=np.float32) * 10.0).astype(np.float32)
    w[rng.random(shape) < 0.001] = -9999.0
    aw = np.abs(w)
    outl = (np.array([1450, 300], dtype=np.int32), np.array([2900, 1700], dtype=np.int32))
    for x, y, nm in zip(ctx.gridnet(p, -32768, dx, dy), oracle.gridnet(p, -32768, dx, dy), ("plen", "tlen", "gord")):
        same(np.asarray(x), np.asarray(y), nm)
    mask = rng.integers(0, 10, shape).astype(np.int32)
    for x, y, nm in zip(ctx.gridnet(p, -32768, dx, dy, mask=mask, thresh=2, outlets=outl), oracle.gridnet(p, -32768, dx, dy, mask=mask, thresh=2, outlets=outl),
                        ("plen (mask, outlets)", "tlen", "gord")):
        same(np.asarray(x), np.asarray(y), nm)
    dm = (0.9 + 0.1 * rng.random(shape, dtype=np.float32)).astype(np.float32)
    sca_o = oracle.areadinf(ang, dx=dx, dy=dy, weights=aw, contcheck=False, outlets=outl)
    dsca_o = oracle.dinfdecayaccum(ang, dm, dx=dx, dy=dy, weights=aw)
    same(ctx.areadinf(ang, dx=dx, dy=dy, weights=aw, contcheck=False, outlets=outl), sca_o, "sca, weights + outlets")
    same(ctx.dinfdecayaccum(ang, dm, dx=dx, dy=dy, weights=aw), dsca_o, "dsca")
    monkeypatch.setenv("TDX_DINF_WALK", "1")
    same(ctx.areadinf(ang, dx=dx, dy=dy, weights=aw, contcheck=False, outlets=outl), sca_o, "sca (walk), weights + outlets")
    same(ctx.dinfdecayaccum(ang, dm, dx=dx, dy=dy, weights=aw), dsca_o, "dsca (walk)")
    monkeypatch.delenv("TDX_DINF_WALK")
    dg = (rng.random(shape) < 0.003).astype(np.int32)
    same(ctx.dinfupdependence(ang, dg, dx=dx, dy=dy), oracle.dinfupdependence(ang, dg, dx=dx, dy=dy), "dep")
    for x, y, nm in zip(ctx.dinfrevaccum(ang, w, dx=dx, dy=dy), oracle.dinfrevaccum(ang, w, dx=dx, dy=dy), ("racc", "dmax")):
        same(x, y, nm)
    q = (0.5 + rng.random(shape, dtype=np.float32)).astype(np.float32)
    same(ctx.dinfconclimaccum(ang, dm, dg.astype(np.int16), q, csol=1.5, dx=dx, dy=dy),
         oracle.dinfconclimaccum(ang, dm, dg.astype(np.int16), q, csol=1.5, dx=dx, dy=dy), "ctpt")
    tc = (rng.random(shape, dtype=np.float32) * 80).astype(np.float32)
    for x, y, nm in zip(ctx.dinftranslimaccum(ang, aw, tc, cs=dm, dx=dx, dy=dy, contcheck=False, outlets=outl),
                        oracle.dinftranslimaccum(ang, aw, tc, cs=dm, dx=dx, dy=dy, contcheck=False, outlets=outl), ("tla", "tdep", "ctpt")):
        same(x, y, nm)
