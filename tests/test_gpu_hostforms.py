"""The host form of every library call (numpy arrays: upload, tdx_x_dev, download) against its device form (torch tensors holding the same
bits) on one 90 x 70 raster - one full 64 x 64 tile and ragged edges both ways, so that a wrong element size or a swapped scratch slot
shows.  Every tool with optional rasters runs with all of them and with none.  The outputs are equal bit for bit, NaN payloads included.
No reference is involved: the two forms run the same kernels on the same inputs."""
import numpy as np
import pytest

import downstream as D
import hand_model
import pathological

NY, NX = 90, 70
DX, DY = 30.0, 40.0
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inp(ctx, oracle):
    """The upstream rasters of a fractal DEM with a nodata corner (from the host forms themselves) and the downstream tools' inputs of
    tests/downstream.py, tests/hand_model.py; never written after this."""
    dem = pathological.fractal(oracle, NY, NX, seed=11)
    dem[:5, :7] = pathological.NODATA
    fel = ctx.pitremove(dem, pathological.NODATA)
    p, sd8 = ctx.d8flowdir(fel, D.FEL_ND, DX, DY)
    ang, slp = ctx.dinfflowdir(fel, D.FEL_ND, DX, DY)
    ad8 = ctx.aread8(p, D.P_ND, contcheck=False)
    sca = ctx.areadinf(ang, D.ANG_ND, DX, DY, contcheck=False)
    inp = D.extras(dict(dem=dem, fel=fel, p=p, sd8=sd8, ang=ang, slp=slp, ad8=ad8, sca=sca), seed=23)
    inp["ass"] = D.late_sources((NY, NX), np.random.default_rng(29))
    inp["catch"] = hand_model.voronoi(NY, NX, 6, seed=31)
    inp["hand"] = ctx.dinfdistdown(ang, inp["src16"], inp["feld"], stat="ave", kind="v", dx=DX, dy=DY)
    for a in inp.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return inp


IDS = np.array([3, 1, 6, 40, 2], np.int32)
STAGES = [0.0, 0.5, 2.0, 8.0]
DEPTHS = np.array([1.5, 0.25, 4.0, 1.0, -1.0], np.float32)

# tool -> f(ctx, r, opt): r(key) is the raster inp[key] on the side under test, opt: every optional raster present / absent
TOOLS = {
    "pitremove": lambda c, r, opt: c.pitremove(r("dem"), pathological.NODATA, mask=r("dgs") if opt else None),
    "d8flowdir": lambda c, r, opt: c.d8flowdir(r("fel"), D.FEL_ND, DX, DY, want_slope=opt)[:1 + opt],
    "dinfflowdir": lambda c, r, opt: c.dinfflowdir(r("fel"), D.FEL_ND, DX, DY),
    "aread8": lambda c, r, opt: c.aread8(r("p"), D.P_ND, weights=r("wpos") if opt else None, contcheck=not opt, outlets=r.outlets if opt else None),
    "d8flowpathextremeup": lambda c, r, opt: c.d8flowpathextremeup(r("p"), r("sa"), D.P_ND, contcheck=not opt, outlets=r.outlets if opt else None),
    "gridnet": lambda c, r, opt: c.gridnet(r("p"), D.P_ND, DX, DY, mask=r("gmask") if opt else None, thresh=D.GN_THRESH, outlets=r.outlets if opt else None),
    "threshold": lambda c, r, opt: c.threshold(r("ad8"), D.SSA_THRESH, -1.0, mask=r("tmask") if opt else None),
    "areadinf": lambda c, r, opt: c.areadinf(r("ang"), D.ANG_ND, DX, DY, weights=r("wpos") if opt else None, contcheck=not opt, outlets=r.outlets if opt else None),
    "dinfdecayaccum": lambda c, r, opt: c.dinfdecayaccum(r("ang"), r("dm"), dx=DX, dy=DY, weights=r("wpos") if opt else None, contcheck=not opt,
                                                          outlets=r.outlets if opt else None),
    "dinfupdependence": lambda c, r, opt: c.dinfupdependence(r("ang"), r("dg"), dx=DX, dy=DY),
    "dinfrevaccum": lambda c, r, opt: c.dinfrevaccum(r("ang"), r("w"), dx=DX, dy=DY),
    "dinfconclimaccum": lambda c, r, opt: c.dinfconclimaccum(r("ang"), r("dm"), r("dgs"), r("q"), csol=D.CSOL, dx=DX, dy=DY, contcheck=not opt,
                                                              outlets=r.outlets if opt else None),
    "dinftranslimaccum": lambda c, r, opt: c.dinftranslimaccum(r("ang"), r("tsup"), r("tc"), r("cs") if opt else None, dx=DX, dy=DY, contcheck=not opt,
                                                                outlets=r.outlets if opt else None)[:2 + opt],
    # with: the surface distance reads fel and the weights; without: the horizontal one reads neither
    "dinfdistdown": lambda c, r, opt: c.dinfdistdown(r("ang"), r("src16"), r("feld") if opt else None, stat="max", kind="s" if opt else "h",
                                                      weights=r("w") if opt else None, dx=DX, dy=DY),
    "dinfdistup": lambda c, r, opt: c.dinfdistup(r("ang"), r("feld") if opt else None, stat="min", kind="s" if opt else "h", weights=r("w") if opt else None,
                                                  dx=DX, dy=DY),
    "retlimflow": lambda c, r, opt: c.retlimflow(r("ang"), r("wpos"), r("q"), dx=DX, dy=DY),
    "dinfavalanche": lambda c, r, opt: c.dinfavalanche(r("ang"), r("feld"), r("ass"), thresh=0.2, alpha=1.0, dx=DX, dy=DY),
    "d8hdisttostrm": lambda c, r, opt: c.d8hdisttostrm(r("p"), r("src32"), 1, dx=DX, dy=DY, src_nodata=D.SRC_ND),
    "d8vdisttostrm": lambda c, r, opt: c.d8vdisttostrm(r("p"), r("feld"), r("src32"), 1, src_nodata=D.SRC_ND),
    "gagewatershed": lambda c, r, opt: c.gagewatershed(r("p"), r.gauges),
    "flowdircond": lambda c, r, opt: c.flowdircond(r("p"), r("feld"), z_nodata=D.FEL_ND),
    "slopeavedown": lambda c, r, opt: c.slopeavedown(r("p"), r("feld"), 2.5 * DX, dx=DX, dy=DY, fel_nodata=D.FEL_ND),
    "catchhydrogeo": lambda c, r, opt: c.catchhydrogeo(r("hand"), r("catch"), r("slp"), IDS, STAGES, dx=DX, dy=DY),
    "inundepth": lambda c, r, opt: c.inundepth(r("hand"), r("catch"), IDS, DEPTHS, mask=r("dgs") if opt else None, area=opt, dx=DX, dy=DY)[:1 + opt],
}
WITH_OPTIONS = ("pitremove", "d8flowdir", "aread8", "d8flowpathextremeup", "gridnet", "threshold", "areadinf", "dinfdecayaccum", "dinfconclimaccum",
                "dinftranslimaccum", "dinfdistdown", "dinfdistup", "inundepth")
CASES = [(t, opt) for t in TOOLS for opt in ((True, False) if t in WITH_OPTIONS else (False,))]


class Rasters:
    """inp's rasters as numpy arrays (host form) or as device tensors with the same bits (device form); outlets and gauges are host lists for both."""

    def __init__(self, inp, device):
        self.inp, self.device, self.outlets, self.gauges = inp, device, inp["outlets"], inp["gauges"]

    def __call__(self, key):
        if self.device is None:
            return self.inp[key]
        import torch

        return torch.from_numpy(self.inp[key].copy()).to(f"cuda:{self.device}")


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_every_tool_is_covered():
    import taudem_amd

    assert len(TOOLS) == 24 and all(hasattr(taudem_amd.Context, t) for t in TOOLS)
    lib = taudem_amd.load()
    assert all(hasattr(lib, f"tdx_{t}") and hasattr(lib, f"tdx_{t}_dev") for t in TOOLS)


@pytest.mark.parametrize("tool,opt", CASES, ids=[t + ("-with" if o else "-without" if t in WITH_OPTIONS else "") for t, o in CASES])
def test_host_form_equals_device_form(ctx, inp, tool, opt):
    host = TOOLS[tool](ctx, Rasters(inp, None), opt)
    dev = TOOLS[tool](ctx, Rasters(inp, ctx.device), opt)
    host, dev = (x if isinstance(x, tuple) else (x,) for x in (host, dev))
    assert len(host) == len(dev) and len(host) >= 1
    for k, (h, d) in enumerate(zip(host, dev)):
        assert isinstance(h, np.ndarray) and h.size > 0
        hb, db = _bits(h), _bits(d)
        assert hb.shape == db.shape and hb.dtype == db.dtype
        assert np.array_equal(hb, db), f"{tool}, output {k}: {int((hb != db).sum())} of {hb.size} values differ between the host form and the device form"
