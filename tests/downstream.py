"""Every tool downstream of the flow directions on one raster, three ways with the same inputs and the same keys:

    derive(oracle, dem, dx, dy, seed, cut_rows)     the oracle's fel / p / sd8 / ang / slp / ad8 / sca of a DEM and the extra inputs the
                                                    downstream tools take, drawn deterministically from `seed` (extras())
    Restate(dirpath, oracle)                        the pinned restatements (oracle/taudem_oracle.c, tests/{distdown,distup,d8rev})
    reference(R, inp, dx, dy, i)                    {key: raster} of the restatements (gagewatershed's -id text under "gw_id")
    single(ctx, inp, dx, dy, i)                     the same through the one-device entry points
    strip(pipe, put, inp, sdx, sdy, y0, y1, i)      the same through the strip entry points on the strip [y0, y1) (owned rows only)

The five dependency-sweep tools that came after those - RetLimFlow, DinfAvalanche, FlowDirCond, D8VDistToStrm, SlopeAveDown - have the same
four forms under names of their own (extras_late, reference_late, single_late, strip_late, compare_late: see "the late tools" below), with
inputs from a generator of their own, so that every input extras() draws keeps its bits and a failure names the new tool.

`i` picks the distance modes: DinfDistDown / DinfDistUp run two of the 12 (stat, kind) pairs each, rotating with i, so that every
pair comes up across consecutive values of i; the -nc / -wg / -thresh variants rotate the same way.  The degenerate source sets (no
stream cell, every valid cell a stream cell) run on every raster.  The flow directions come from the oracle, so a failure is located
in the tool that is compared and not upstream of it.
"""
import numpy as np

import aval_model
import d8last_model
import d8rev_model
import distdown_model
import distup_model

NODATA = -9999.0
ANG_ND = -3.402823466e38
FEL_ND = -3.0e38
P_ND = -32768
SRC_ND = -2147483647          # int32 -src nodata of D8HDistToStrm
MODES = [(s, k) for s in distdown_model.STATS for k in distdown_model.KINDS]   # the 12 -m forms
GN_THRESH = 4
SSA_THRESH = 25.0
CSOL = 2.5
NO_STRIP_FORM = ("thr", "thr_m")   # Threshold is a cell-wise map without a strip entry point


def dd_variants(i):
    """[(stat, kind, suffix)] of the DinfDistDown runs for index i (suffix '' / '_nc' / '_wg')."""
    return [MODES[i % 12] + (("", "_nc", "_wg")[i % 3],), MODES[(i + 7) % 12] + (("_wg", "", "_nc")[i % 3],)]


def du_variants(i):
    """[(stat, kind, suffix)] of the DinfDistUp runs for index i (suffix '' / '_nc' / '_wg' / '_t')."""
    return [MODES[(i + 3) % 12] + (("", "_nc", "_wg", "_t")[i % 4],), MODES[(i + 10) % 12] + (("_t", "_wg", "", "_nc")[i % 4],)]


def _pick(rng, cand, k):
    cand = np.asarray(cand)
    return [int(c) for c in rng.choice(cand, min(k, cand.size), replace=False)] if cand.size else []


def derive(oracle, dem, dx, dy, seed, cut_rows=()):
    fel = oracle.pitremove(dem, NODATA)
    p, sd8, _ = oracle.d8flowdir(fel, FEL_ND, dx, dy)
    ang, slp, _ = oracle.dinfflowdir(fel, FEL_ND, dx, dy)
    ad8 = oracle.aread8(p, P_ND, contcheck=False)
    sca = oracle.areadinf(ang, ANG_ND, dx, dy, contcheck=False)
    return extras(dict(fel=fel, p=p, sd8=sd8, ang=ang, slp=slp, ad8=ad8, sca=sca), seed, cut_rows)


def extras(inp, seed, cut_rows=()):
    """inp: fel, p, sd8, ang, slp, ad8 (-nc), sca (-nc) of one raster; adds the downstream tools' other inputs, drawn from `seed`."""
    fel, p, sd8, ang, ad8, sca = (inp[k] for k in ("fel", "p", "sd8", "ang", "ad8", "sca"))
    ny, nx = p.shape
    rng = np.random.default_rng(seed)
    r = lambda: rng.random((ny, nx))  # noqa: E731
    # distance tools: fel with a few nodata cells under valid angles; stream cells = top 10 % of the D-infinity area, a few nodata
    feld = fel.copy()
    feld[r() < 0.003] = FEL_ND
    inp["feld"] = feld
    valid = (ang > -1e30) & (sca >= 0)         # (AreaDinf's nodata is -1)
    src = np.zeros((ny, nx), np.int16)
    if valid.any():
        src[valid & (sca >= np.quantile(sca[valid], 0.9))] = 1
    src[r() < 0.003] = -32768
    inp["src16"] = src
    inp["src16_all"] = np.where(valid, 1, 0).astype(np.int16)
    # weights in steps of 1/8, a few negative, a few nodata (DinfDistDown / DinfDistUp -wg, DinfRevAccum, weighted DinfDecayAccum)
    w = (0.5 + rng.integers(0, 17, (ny, nx)) / 8.0).astype(np.float32)
    neg = r() < 0.05
    w[neg] = -w[neg]
    w[r() < 0.01] = np.float32(NODATA)
    inp["w"] = w
    inp["wpos"] = np.abs(w).astype(np.float32)
    inp["dg"] = (r() < 0.02).astype(np.int32)
    # (values on coarse grids of steps: the fixtures of tests/golden/patho_*.npz stay small)
    dm = (0.9 + rng.integers(0, 26, (ny, nx)) / 256.0).astype(np.float32)
    dm[r() < 0.003] = np.float32(NODATA)
    inp["dm"] = dm
    q = (0.5 + rng.integers(0, 64, (ny, nx)) / 16.0).astype(np.float32)
    q[r() < 0.004] = 0.0
    q[r() < 0.002] = np.float32(NODATA)
    inp["q"] = q
    inp["dgs"] = (r() < 0.02).astype(np.int16)
    for k, hi in (("tsup", 32), ("tc", 96), ("cs", 16)):
        a = (rng.integers(0, hi, (ny, nx)) / 16.0).astype(np.float32)
        a[r() < 0.003] = np.float32(NODATA)
        inp[k] = a
    # D8 side: int32 stream cells (top 6 % of AreaD8, nodata holes), the contributing area as int32, the gridnet mask, an sa grid with ties
    # and signed zeros (the extreme's comparison decides which zero survives) that keeps sd8's non-finite values
    ad8i = np.where(ad8 < -0.5, SRC_ND, np.rint(ad8)).astype(np.int32)
    dvalid = ad8i != SRC_ND
    s32 = np.zeros((ny, nx), np.int32)
    if dvalid.any():
        s32[dvalid & (ad8i >= np.quantile(ad8i[dvalid], 0.94))] = 1
    s32[r() < 0.003] = SRC_ND
    inp["src32"] = s32
    inp["src32_none"] = np.where(r() < 0.01, SRC_ND, 0).astype(np.int32)
    inp["ad8i"] = ad8i
    inp["gmask"] = np.where(ad8 < 0, -7, ad8).astype(np.int32)
    sa = (rng.integers(-4, 5, (ny, nx)) * 0.5).astype(np.float32)
    sa[sa == 0] = np.where(r()[sa == 0] < 0.5, np.float32(-0.0), np.float32(0.0))
    sa = np.where(np.isfinite(sd8), sa, sd8).astype(np.float32)
    inp["sa"] = sa
    inp["tmask"] = np.where(r() < 0.2, np.float32(-0.5), np.float32(0.5)).astype(np.float32)
    # outlets (columns, rows): large-area cells with a direction, plus the largest of each cut row
    cut = [int(y) for y in cut_rows if 0 <= y < ny]
    dflat = np.flatnonzero(p.ravel() != P_ND)
    big = dflat[np.argsort(ad8.ravel()[dflat])[-200:]] if dflat.size else dflat
    picks = _pick(rng, big, 4)
    for y in cut:
        row = np.where(p[y] != P_ND, ad8[y], -np.inf)
        if np.isfinite(row.max()):
            picks.append(y * nx + int(np.argmax(row)))
    inp["outlets"] = (np.array([c % nx for c in picks], np.int32), np.array([c // nx for c in picks], np.int32))
    # gauges: the outlets, one on a cell without a direction, a second one on a taken cell, one off the raster; shuffled ids
    gp = list(picks)
    nod = np.flatnonzero(p.ravel() == P_ND)
    gp += _pick(rng, nod, 1)
    cols = [c % nx for c in gp] + ([gp[0] % nx] if gp else []) + [nx + 5]
    rws = [c // nx for c in gp] + ([gp[0] // nx] if gp else []) + [ny // 2]
    ids = (rng.permutation(10 * len(cols))[:len(cols)] + 1).astype(np.int32)
    inp["gauges"] = (np.array(cols, np.int32), np.array(rws, np.int32), ids)
    return inp


class Restate:
    def __init__(self, dirpath, oracle):
        self.o = oracle
        self.dd = distdown_model.compile(dirpath)
        self.du = distup_model.compile(dirpath)
        self.rev = d8rev_model.compile(dirpath)
        self.aval = aval_model.compile(dirpath)
        self.last = d8last_model.compile(dirpath)


def _dd_args(inp, sfx):
    return dict(weights=inp["w"] if sfx == "_wg" else None, contcheck=sfx != "_nc")


def _du_args(inp, sfx):
    return dict(weights=inp["w"] if sfx == "_wg" else None, contcheck=sfx != "_nc", thresh=distup_model.THRESH if sfx == "_t" else 0.0)


def reference(R, inp, dx, dy, i):
    o, out = R.o, {}
    ang, p = inp["ang"], inp["p"]
    out["dep"] = o.dinfupdependence(ang, inp["dg"], dx=dx, dy=dy)
    out["racc"], out["dmax"] = o.dinfrevaccum(ang, inp["w"], dx=dx, dy=dy)
    out["dsca"] = o.dinfdecayaccum(ang, inp["dm"], dx=dx, dy=dy, weights=inp["wpos"], contcheck=True)
    out["dsca_o"] = o.dinfdecayaccum(ang, inp["dm"], dx=dx, dy=dy, contcheck=False, outlets=inp["outlets"])
    out["ctpt"] = o.dinfconclimaccum(ang, inp["dm"], inp["dgs"], inp["q"], csol=CSOL, dx=dx, dy=dy)
    out["ctpt_o"] = o.dinfconclimaccum(ang, inp["dm"], inp["dgs"], inp["q"], dx=dx, dy=dy, contcheck=False, outlets=inp["outlets"])
    out["tla"], out["tdep"], _ = o.dinftranslimaccum(ang, inp["tsup"], inp["tc"], dx=dx, dy=dy)
    out["tla_cs"], out["tdep_cs"], out["tctpt_cs"] = o.dinftranslimaccum(ang, inp["tsup"], inp["tc"], inp["cs"], dx=dx, dy=dy, contcheck=False,
                                                                         outlets=inp["outlets"])
    for st, kd, sfx in dd_variants(i):
        out[f"dd_{st}_{kd}{sfx}"] = R.dd(ang, inp["src16"], inp["feld"], stat=st, kind=kd, dxc=dx, dyc=dy, **_dd_args(inp, sfx))
    out["dd_ave_h_none"] = R.dd(ang, np.zeros_like(inp["src16"]), inp["feld"], stat="ave", kind="h", dxc=dx, dyc=dy)
    out["dd_min_s_all"] = R.dd(ang, inp["src16_all"], inp["feld"], stat="min", kind="s", dxc=dx, dyc=dy)
    for st, kd, sfx in du_variants(i):
        out[f"du_{st}_{kd}{sfx}"] = R.du(ang, inp["feld"], stat=st, kind=kd, dxc=dx, dyc=dy, **_du_args(inp, sfx))
    out["dist"] = R.rev.dist(p, inp["src32"], 1, dx, dy, src_nodata=SRC_ND)
    out["dist_none"] = R.rev.dist(p, inp["src32_none"], 1, dx, dy, src_nodata=SRC_ND)
    out["dist_ad8"] = R.rev.dist(p, inp["ad8i"], 40, dx, dy, src_nodata=SRC_ND)
    out["gw"], out["gw_id"] = R.rev.gage(p, *inp["gauges"])
    out["plen"], out["tlen"], out["gord"] = o.gridnet(p, P_ND, dx, dy)
    out["plen_m"], out["tlen_m"], out["gord_m"] = o.gridnet(p, P_ND, dx, dy, mask=inp["gmask"], thresh=GN_THRESH)
    out["plen_o"], out["tlen_o"], out["gord_o"] = o.gridnet(p, P_ND, dx, dy, outlets=inp["outlets"])
    out["xup_max"] = o.d8flowpathextremeup(p, inp["sa"], P_ND, usemax=True, contcheck=True)
    out["xup_min_nc"] = o.d8flowpathextremeup(p, inp["sa"], P_ND, usemax=False, contcheck=False)
    out["xup_max_o"] = o.d8flowpathextremeup(p, inp["sa"], P_ND, usemax=True, contcheck=False, outlets=inp["outlets"])
    out["thr"] = o.threshold(inp["ad8"], SSA_THRESH, -1.0)
    out["thr_m"] = o.threshold(inp["ad8"], SSA_THRESH, -1.0, mask=inp["tmask"])
    return out


def single(ctx, inp, dx, dy, i):
    """The one-device entry points; also Threshold (which has no strip form)."""
    out = {}
    ang, p = inp["ang"], inp["p"]
    out["dep"] = ctx.dinfupdependence(ang, inp["dg"], dx=dx, dy=dy)
    out["racc"], out["dmax"] = ctx.dinfrevaccum(ang, inp["w"], dx=dx, dy=dy)
    out["dsca"] = ctx.dinfdecayaccum(ang, inp["dm"], dx=dx, dy=dy, weights=inp["wpos"], contcheck=True)
    out["dsca_o"] = ctx.dinfdecayaccum(ang, inp["dm"], dx=dx, dy=dy, contcheck=False, outlets=inp["outlets"])
    out["ctpt"] = ctx.dinfconclimaccum(ang, inp["dm"], inp["dgs"], inp["q"], csol=CSOL, dx=dx, dy=dy)
    out["ctpt_o"] = ctx.dinfconclimaccum(ang, inp["dm"], inp["dgs"], inp["q"], dx=dx, dy=dy, contcheck=False, outlets=inp["outlets"])
    out["tla"], out["tdep"], _ = ctx.dinftranslimaccum(ang, inp["tsup"], inp["tc"], dx=dx, dy=dy)
    out["tla_cs"], out["tdep_cs"], out["tctpt_cs"] = ctx.dinftranslimaccum(ang, inp["tsup"], inp["tc"], inp["cs"], dx=dx, dy=dy, contcheck=False,
                                                                           outlets=inp["outlets"])
    for st, kd, sfx in dd_variants(i):
        out[f"dd_{st}_{kd}{sfx}"] = ctx.dinfdistdown(ang, inp["src16"], inp["feld"], stat=st, kind=kd, dx=dx, dy=dy, **_dd_args(inp, sfx))
    out["dd_ave_h_none"] = ctx.dinfdistdown(ang, np.zeros_like(inp["src16"]), inp["feld"], stat="ave", kind="h", dx=dx, dy=dy)
    out["dd_min_s_all"] = ctx.dinfdistdown(ang, inp["src16_all"], inp["feld"], stat="min", kind="s", dx=dx, dy=dy)
    for st, kd, sfx in du_variants(i):
        out[f"du_{st}_{kd}{sfx}"] = ctx.dinfdistup(ang, inp["feld"], stat=st, kind=kd, dx=dx, dy=dy, **_du_args(inp, sfx))
    out["dist"] = ctx.d8hdisttostrm(p, inp["src32"], 1, dx=dx, dy=dy, src_nodata=SRC_ND)
    out["dist_none"] = ctx.d8hdisttostrm(p, inp["src32_none"], 1, dx=dx, dy=dy, src_nodata=SRC_ND)
    out["dist_ad8"] = ctx.d8hdisttostrm(p, inp["ad8i"], 40, dx=dx, dy=dy, src_nodata=SRC_ND)
    out["gw"], table = ctx.gagewatershed(p, inp["gauges"])
    out["gw_id"] = d8rev_model.table_text(table)
    out["plen"], out["tlen"], out["gord"] = ctx.gridnet(p, P_ND, dx, dy)
    out["plen_m"], out["tlen_m"], out["gord_m"] = ctx.gridnet(p, P_ND, dx, dy, mask=inp["gmask"], thresh=GN_THRESH)
    out["plen_o"], out["tlen_o"], out["gord_o"] = ctx.gridnet(p, P_ND, dx, dy, outlets=inp["outlets"])
    out["xup_max"] = ctx.d8flowpathextremeup(p, inp["sa"], P_ND, usemax=True, contcheck=True)
    out["xup_min_nc"] = ctx.d8flowpathextremeup(p, inp["sa"], P_ND, usemax=False, contcheck=False)
    out["xup_max_o"] = ctx.d8flowpathextremeup(p, inp["sa"], P_ND, usemax=True, contcheck=False, outlets=inp["outlets"])
    out["thr"] = ctx.threshold(inp["ad8"], SSA_THRESH, -1.0)
    out["thr_m"] = ctx.threshold(inp["ad8"], SSA_THRESH, -1.0, mask=inp["tmask"])
    return out


def strip(pipe, put, inp, sdx, sdy, y0, y1, i):
    """The strip entry points on [y0, y1): put(array) -> the strip array of a global raster; sdx / sdy the strip's rows (strip_rows).
    Returns the owned rows as numpy arrays; "gw_id" is this rank's id table as text."""
    import torch

    ang, p = put(inp["ang"]), put(inp["p"])
    lo = pipe.local_outlets(inp["outlets"][0], inp["outlets"][1], y0)
    gl = pipe.local_outlets(inp["gauges"][0], inp["gauges"][1], y0)
    out = {}
    out["dep"], _ = pipe.dinfupdependence(ang, put(inp["dg"]), dx=sdx, dy=sdy)
    out["racc"], out["dmax"], _ = pipe.dinfrevaccum(ang, put(inp["w"]), dx=sdx, dy=sdy)
    dm = put(inp["dm"])
    out["dsca"], _ = pipe.dinfdecayaccum(ang, dm, dx=sdx, dy=sdy, weights=put(inp["wpos"]), contcheck=True)
    out["dsca_o"], _ = pipe.dinfdecayaccum(ang, dm, dx=sdx, dy=sdy, contcheck=False, outlets=lo)
    dgs, q = put(inp["dgs"]), put(inp["q"])
    out["ctpt"], _ = pipe.dinfconclimaccum(ang, dm, dgs, q, csol=CSOL, dx=sdx, dy=sdy)
    out["ctpt_o"], _ = pipe.dinfconclimaccum(ang, dm, dgs, q, dx=sdx, dy=sdy, contcheck=False, outlets=lo)
    tsup, tc = put(inp["tsup"]), put(inp["tc"])
    out["tla"], out["tdep"], _, _ = pipe.dinftranslimaccum(ang, tsup, tc, dx=sdx, dy=sdy)
    out["tla_cs"], out["tdep_cs"], out["tctpt_cs"], _ = pipe.dinftranslimaccum(ang, tsup, tc, put(inp["cs"]), dx=sdx, dy=sdy, contcheck=False, outlets=lo)
    feld, w = put(inp["feld"]), put(inp["w"])
    for st, kd, sfx in dd_variants(i):
        out[f"dd_{st}_{kd}{sfx}"], _ = pipe.dinfdistdown(ang, put(inp["src16"]), feld, stat=st, kind=kd, dx=sdx, dy=sdy,
                                                         weights=w if sfx == "_wg" else None, contcheck=sfx != "_nc")
    out["dd_ave_h_none"], _ = pipe.dinfdistdown(ang, put(np.zeros_like(inp["src16"])), feld, stat="ave", kind="h", dx=sdx, dy=sdy)
    out["dd_min_s_all"], _ = pipe.dinfdistdown(ang, put(inp["src16_all"]), feld, stat="min", kind="s", dx=sdx, dy=sdy)
    for st, kd, sfx in du_variants(i):
        out[f"du_{st}_{kd}{sfx}"], _ = pipe.dinfdistup(ang, feld, stat=st, kind=kd, dx=sdx, dy=sdy, weights=w if sfx == "_wg" else None,
                                                       contcheck=sfx != "_nc", thresh=distup_model.THRESH if sfx == "_t" else 0.0)
    out["dist"], _ = pipe.d8hdisttostrm(p, put(inp["src32"]), 1, dx=sdx, dy=sdy, src_nodata=SRC_ND)
    out["dist_none"], _ = pipe.d8hdisttostrm(p, put(inp["src32_none"]), 1, dx=sdx, dy=sdy, src_nodata=SRC_ND)
    out["dist_ad8"], _ = pipe.d8hdisttostrm(p, put(inp["ad8i"]), 40, dx=sdx, dy=sdy, src_nodata=SRC_ND)
    out["gw"], table, _ = pipe.gagewatershed(p, (gl[0], gl[1], inp["gauges"][2]))
    out["plen"], out["tlen"], out["gord"], _ = pipe.gridnet(p, P_ND, sdx, sdy)
    out["plen_m"], out["tlen_m"], out["gord_m"], _ = pipe.gridnet(p, P_ND, sdx, sdy, mask=put(inp["gmask"]), thresh=GN_THRESH)
    out["plen_o"], out["tlen_o"], out["gord_o"], _ = pipe.gridnet(p, P_ND, sdx, sdy, outlets=lo)
    sa = put(inp["sa"])
    out["xup_max"], _ = pipe.d8flowpathextremeup(p, sa, P_ND, usemax=True, contcheck=True)
    out["xup_min_nc"], _ = pipe.d8flowpathextremeup(p, sa, P_ND, usemax=False, contcheck=False)
    out["xup_max_o"], _ = pipe.d8flowpathextremeup(p, sa, P_ND, usemax=True, contcheck=False, outlets=lo)
    torch.cuda.synchronize()
    res = {k: v[1:y1 - y0 + 1].cpu().numpy() for k, v in out.items()}
    res["gw_id"] = d8rev_model.table_text(table)
    return res


def reference_upstream(oracle, dem, inp, dx, dy):
    """The strip-capable tools upstream of the directions (what strip_upstream computes), from the restatement."""
    o, out = oracle, {}
    out["fel"], out["p"], out["sd8"], out["ang"], out["slp"] = inp["fel"], inp["p"], inp["sd8"], inp["ang"], inp["slp"]
    out["ad8"] = o.aread8(inp["p"], P_ND, contcheck=True)
    out["ad8_w"] = o.aread8(inp["p"], P_ND, weights=inp["wpos"], contcheck=False)
    out["ad8_o"] = o.aread8(inp["p"], P_ND, contcheck=False, outlets=inp["outlets"])
    out["sca"] = o.areadinf(inp["ang"], ANG_ND, dx, dy, contcheck=True)
    out["sca_o"] = o.areadinf(inp["ang"], ANG_ND, dx, dy, weights=inp["wpos"], contcheck=False, outlets=inp["outlets"])
    return out


def strip_upstream(pipe, put, dem, inp, sdx, sdy, y0, y1):
    """PitRemove, D8FlowDir, DinfFlowDir from the DEM, AreaD8 / AreaDinf from the oracle's directions, on the strip [y0, y1)."""
    import torch

    out = {}
    out["fel"], _ = pipe.pitremove(put(dem), NODATA)
    out["p"], out["sd8"], _ = pipe.d8flowdir(put(inp["fel"]), FEL_ND, sdx, sdy)
    out["ang"], out["slp"], _ = pipe.dinfflowdir(put(inp["fel"]), FEL_ND, sdx, sdy)
    p, ang, w = put(inp["p"]), put(inp["ang"]), put(inp["wpos"])
    lo = pipe.local_outlets(inp["outlets"][0], inp["outlets"][1], y0)
    out["ad8"], _ = pipe.aread8(p, P_ND, contcheck=True)
    out["ad8_w"], _ = pipe.aread8(p, P_ND, weights=w, contcheck=False)
    out["ad8_o"], _ = pipe.aread8(p, P_ND, contcheck=False, outlets=lo)
    out["sca"], _ = pipe.areadinf(ang, ANG_ND, sdx, sdy, contcheck=True)
    out["sca_o"], _ = pipe.areadinf(ang, ANG_ND, sdx, sdy, weights=w, contcheck=False, outlets=lo)
    torch.cuda.synchronize()
    return {k: v[1:y1 - y0 + 1].cpu().numpy() for k, v in out.items()}


def compare(got, ref, what):
    """Every key of got against ref, bit for bit (ids as text); returns the list of failures."""
    from conftest import bits_equal, describe_diff

    bad = [f"{what}: {k} not computed" for k in sorted(set(ref) - set(got) - set(NO_STRIP_FORM))]
    for k in got:
        r = ref[k]
        if k == "gw_id":
            if got[k] != r:
                bad.append(f"{what}: gagewatershed -id text {got[k]!r} vs {r!r}")
        elif not bits_equal(np.asarray(got[k]), r):
            bad.append(describe_diff(np.asarray(got[k]), r, f"{what}: {k}"))
    return bad


# ---- the late tools: RetLimFlow, DinfAvalanche, FlowDirCond, D8VDistToStrm, SlopeAveDown ------------------------------------------------
#
#     extras_late(inp, seed, R, dx, dy, i)                 adds wg / rc / z / ass (and the avalanche's cell sizes and geometry) to inp
#     reference_late(R, inp, dx, dy, i)                    {key: raster} of the restatements, "taint_path" / "taint_direct" beside them
#     single_late(ctx, inp, dx, dy, i)                     the same through the one-device entry points
#     strip_late(pipe, put, inp, sdx, sdy, y0, y1, ny_total, niter_of_whole, i)    the same on the strip [y0, y1)
#     compare_late(got, ref, what)                         bit for bit; rz / dfs by aval_model.compare_aval
#
# Keys: qrl; zfdc; vd, vd_none, vd_ad8 (thresh 40); slpd_a, slpd_b (two dn values rotating with i, late_dns); rz_path, dfs_path, rz_direct,
# dfs_direct at aval_model.DEFAULT and rz_path_lo, dfs_path_lo, rz_direct_lo, dfs_direct_lo at LOW.
#
# The avalanche never runs on cells like 10 x 12.5 (tests/test_gpu_aval.py: the two orders of one straight and one diagonal step round
# differently, and 10 - 30 % of a runout is a near-tie): constant cell sizes become 30 x 40, whose diagonal of 50 makes every path length
# exact, per-row sizes stay (aval_cells).  The directions are an input like any other, so this changes nothing about what is compared.
# alpha = 18 degrees gives next to no runout on ramps and planes (the sources alone), so both modes also run at alpha = 1 degree (LOW):
# on every raster with constant cells, not in rotation, so that each sloped case has a large runout in both modes whatever its index.
# Per-row sizes run at DEFAULT alone: the fan below a source at alpha = 1 is full of confluences of two paths from that source, whose
# lengths differ in the last bits on rows of unequal sizes (seven of eleven `wild` fuzz rasters found no source seed inside the cap;
# with the restatement alone).  The source cells are chosen so that the RESTATEMENT ALONE keeps
# the tainted share at or below 0.8 x aval_model.MAX_TAINT_SHARE in every run (up to 12 source seeds, as test_gpu_aval._check_aval does);
# compare_aval then asserts the 1 % itself.
#
# -direct mode on ramp_diag / ramp_antidiag: on a plane tilted along the diagonal the straight-line distances from one source to the cells
# of its runout tie in float32 wherever two contributors carry the same source (measured with the restatement alone, density 0.002, six
# source seeds: 12 - 55 % of the runout tainted).  LATE_DIRECT gives those two cases one source cell for their -direct runs, with which
# no cell is tainted (the runouts are in the table of tests/test_gpu_pathological_downstream.py).
LOW = (0.2, 1.0)
LATE_DIRECT = {"ramp_diag": "single", "ramp_antidiag": "single"}
# cells with rz data the path mode must reach at alpha = 1 on tests/pathological.py's sloped rasters (restatement alone, 30 x 40 cells, the
# sources extras_late chooses: ramp_diag 68 646, ramp_antidiag 70 084, ramp_-x 16 024, ramp_x 14 887, ramp_y 13 584, ramp_-y 11 933,
# spiral 9 264, +inf_cells 7 173, nan_cells 7 065, -inf_cells 6 130)
LATE_FLOOR = {k: 5000 for k in ("ramp_x", "ramp_-x", "ramp_y", "ramp_-y", "ramp_diag", "ramp_antidiag", "spiral", "nan_cells", "+inf_cells", "-inf_cells")}
PYTH = (30.0, 40.0)
ASS_DENSITY = 0.002
SOURCE_SEEDS = 12
DN_FACTORS = (0.5, 2.5, 6.2, 12.3)
WG_ND = RC_ND = -9999.0
LATE_BITWISE = ("qrl", "zfdc", "vd", "vd_none", "vd_ad8", "slpd_a", "slpd_b")


def aval_cells(dx, dy, rows=True):
    """The avalanche's cell sizes for a raster whose other tools run at (dx, dy): 30 x 40 for constant cells; per-row sizes stay when `rows`."""
    return (dx, dy) if rows and (np.ndim(dx) or np.ndim(dy)) else PYTH


def aval_runs():
    """[(suffix, direct, (thresh, alpha))]: the path mode and the -direct mode, each at aval_model.DEFAULT and at LOW."""
    return [("_path", False, aval_model.DEFAULT), ("_direct", True, aval_model.DEFAULT), ("_path_lo", False, LOW), ("_direct_lo", True, LOW)]


def late_dns(dx, dy, i):
    """[(key, dn, niter of the whole raster)] of the two SlopeAveDown runs for index i."""
    dxc, dyc = np.atleast_1d(np.asarray(dx, np.float64)), np.atleast_1d(np.asarray(dy, np.float64))
    m = min(abs(float(dxc[dxc.size // 2])), abs(float(dyc[dyc.size // 2])))
    dns = [DN_FACTORS[i % 4] * m, DN_FACTORS[(i + 2) % 4] * m]
    return [(k, dn, d8last_model.niter_of(dn, dx, dy)) for k, dn in zip(("slpd_a", "slpd_b"), dns)]


def late_sources(shape, rng, single=False):
    """ass, int16: source cells at ASS_DENSITY, a quarter as many nodata cells, one 2 x 3 patch of 3s; single: one source cell and nothing else."""
    ny, nx = shape
    ass = np.zeros(shape, np.int16)
    if single:
        ass[int(rng.integers(0, ny)), int(rng.integers(0, nx))] = 1
        return ass
    ass[rng.random(shape) < ASS_DENSITY] = 1
    ass[rng.random(shape) < ASS_DENSITY / 4] = aval_model.ASS_NODATA
    if ass.size > 200:
        y, x = int(rng.integers(0, max(ny - 2, 1))), int(rng.integers(0, max(nx - 3, 1)))
        ass[y:y + 2, x:x + 3] = 3
    return ass


def _aval_ref(R, inp, ass, direct, ta):
    adx, ady = inp["aval_cells"]
    return R.aval.dinfavalanche(inp["ang_a"], inp["feld"], ass, thresh=ta[0], alpha=ta[1], direct=direct, dxc=adx, dyc=ady, geo=inp["aval_geo"])


def _inside(refs):
    return all(t.sum() <= 0.8 * aval_model.MAX_TAINT_SHARE * max(int((rz > -1e30).sum()), 1) for rz, _, t in refs)


def extras_late(inp, seed, R, dx=30.0, dy=30.0, i=0, direct="scattered", floor=0, aval_rows=True):
    """inp: derive()'s / extras()'s dictionary; adds the late tools' inputs, drawn from default_rng([seed, 1]) (and [seed, 1, s] for the
    s-th source seed): nothing extras() draws changes.  dx, dy: the raster's cell sizes (scalars or global rows).  direct: what the -direct
    run gets - "scattered" the sources of the path run, "single" one source cell of its own (inp["ass_direct"]).
    aval_rows=False: the avalanche runs on 30 x 40 cells even where dx, dy are rows (a planar ramp under `wild` rows: every cell of the fan
    below a source is a confluence of two paths from that source, every 11th row repeats its neighbour's sizes, and half the runout is a
    near-tie).  floor: the least number of cells with rz data the path mode must reach at alpha = 1 with the chosen sources (asserted here, with the
    restatement alone, whichever alpha the path run of index i has)."""
    fel, ang = inp["fel"], inp["ang"]
    ny, nx = ang.shape
    rng = np.random.default_rng([seed, 1])
    r = lambda: rng.random((ny, nx))  # noqa: E731
    # runoff / retention in steps of 1/8, blocks where the retention wins, a few nodata cells in both
    wg = (rng.integers(0, 33, (ny, nx)) / 8.0).astype(np.float32)
    rc = (rng.integers(0, 9, (ny, nx)) / 8.0).astype(np.float32)
    for _ in range(max(1, ny * nx // 20000)):
        y, x = int(rng.integers(0, max(ny - 8, 1))), int(rng.integers(0, max(nx - 8, 1)))
        rc[y:y + 10, x:x + 10] += np.float32(30.0)
    wg[r() < 0.0005] = np.float32(WG_ND)
    rc[r() < 0.0005] = np.float32(RC_ND)
    inp["wg"], inp["rc"] = wg, rc
    # z = fel + noise of 3 m in steps of 1/16 (not pit-filled along p: on fel itself FlowDirCond changes nothing); fel's nodata stays
    fel = np.where(fel < -1e30, np.float32(FEL_ND), fel).astype(np.float32)
    noise = np.rint(rng.normal(0.0, 3.0, (ny, nx)) * 16.0) / 16.0
    with np.errstate(invalid="ignore", over="ignore"):
        inp["z"] = np.where(fel > -1e30, (fel + noise).astype(np.float32), fel).astype(np.float32)   # (NaN stays NaN: not > -1e30)
    adx, ady = aval_cells(dx, dy, aval_rows)
    inp["aval_cells"] = (adx, ady)
    if "ang_a" not in inp:   # the avalanche's angles belong to its own cells: the oracle's D-infinity directions of fel on 30 x 40
        inp["ang_a"] = inp["ang"] if adx is dx and ady is dy else R.o.dinfflowdir(inp["fel"], FEL_ND, adx, ady)[0]
    inp["aval_geo"] = aval_model.default_geo(ny, adx, ady)
    inp["aval_direct"] = direct
    runs = [(d, ta) for _, d, ta, _ in _aval_inputs(dict(inp, ass=None, ass_direct=None)) if not d or direct == "scattered"]
    for s in range(SOURCE_SEEDS):
        ass = late_sources((ny, nx), np.random.default_rng([seed, 1, s]))
        if _inside([_aval_ref(R, inp, ass, d, ta) for d, ta in runs]):
            break
    else:
        raise AssertionError(f"no source seed of {SOURCE_SEEDS} keeps the restatement's tainted share within 0.8 x {aval_model.MAX_TAINT_SHARE}")
    inp["ass"] = ass
    if direct == "single":
        for s in range(SOURCE_SEEDS):
            one = late_sources((ny, nx), np.random.default_rng([seed, 2, s]), single=True)
            if _inside([_aval_ref(R, inp, one, True, ta) for _, d, ta, _ in _aval_inputs(dict(inp, ass=None, ass_direct=None)) if d]):
                break
        else:
            raise AssertionError(f"no single source of {SOURCE_SEEDS} keeps the -direct run's tainted share within 0.8 x {aval_model.MAX_TAINT_SHARE}")
        inp["ass_direct"] = one
    if floor:
        rz, _, _ = _aval_ref(R, inp, ass, False, LOW)
        assert int((rz > -1e30).sum()) >= floor, f"path mode at alpha 1: {int((rz > -1e30).sum())} cells with rz data, the floor is {floor}"
    return inp


def _aval_inputs(inp):
    """[(suffix, direct, (thresh, alpha), ass)] of the avalanche runs that inp asks for."""
    out = []
    for sfx, d, ta in aval_runs():
        if ta == LOW and np.ndim(inp["aval_cells"][0]):
            continue
        out.append((sfx, d, ta, inp["ass_direct"] if d and inp["aval_direct"] == "single" else inp["ass"]))
    return out


def aval_taints(R, inp):
    """{"taint" + suffix: mask} of inp's avalanche runs (the restatement's: what compare_aval leaves out and counts)."""
    return {"taint" + sfx: _aval_ref(R, inp, ass, d, ta)[2] for sfx, d, ta, ass in _aval_inputs(inp)}


def reference_late(R, inp, dx, dy, i):
    out = {}
    p, feld = inp["p"], inp["feld"]
    out["qrl"] = R.aval.retlimflow(inp["ang"], inp["wg"], inp["rc"], dxc=dx, dyc=dy)
    out["zfdc"] = R.last.flowdircond(p, inp["z"], FEL_ND)
    out["vd"] = R.last.vdist(p, feld, inp["src32"], 1, src_nodata=SRC_ND)
    out["vd_none"] = R.last.vdist(p, feld, inp["src32_none"], 1, src_nodata=SRC_ND)
    out["vd_ad8"] = R.last.vdist(p, feld, inp["ad8i"], 40, src_nodata=SRC_ND)
    for k, dn, niter in late_dns(dx, dy, i):
        out[k] = R.last.slopeavedown(p, feld, dn, dx, dy, FEL_ND, niter=niter)
    for sfx, d, ta, ass in _aval_inputs(inp):
        out["rz" + sfx], out["dfs" + sfx], out["taint" + sfx] = _aval_ref(R, inp, ass, d, ta)
    return out


def single_late(ctx, inp, dx, dy, i):
    out = {}
    p, feld = inp["p"], inp["feld"]
    out["qrl"] = ctx.retlimflow(inp["ang"], inp["wg"], inp["rc"], dx=dx, dy=dy)
    out["zfdc"] = ctx.flowdircond(p, inp["z"], z_nodata=FEL_ND)
    out["vd"] = ctx.d8vdisttostrm(p, feld, inp["src32"], 1, src_nodata=SRC_ND)
    out["vd_none"] = ctx.d8vdisttostrm(p, feld, inp["src32_none"], 1, src_nodata=SRC_ND)
    out["vd_ad8"] = ctx.d8vdisttostrm(p, feld, inp["ad8i"], 40, src_nodata=SRC_ND)
    for k, dn, niter in late_dns(dx, dy, i):
        out[k] = ctx.slopeavedown(p, feld, dn, dx=dx, dy=dy, fel_nodata=FEL_ND)
    adx, ady = inp["aval_cells"]
    for sfx, d, ta, ass in _aval_inputs(inp):
        out["rz" + sfx], out["dfs" + sfx] = ctx.dinfavalanche(inp["ang_a"], feld, ass, thresh=ta[0], alpha=ta[1], direct=d, dx=adx, dy=ady, geo=inp["aval_geo"])
    return out


def strip_late(pipe, put, inp, sdx, sdy, y0, y1, ny_total, niter_of_whole, i):
    """The strip entry points on [y0, y1).  niter_of_whole: late_dns(dx, dy, i) of the WHOLE raster's rows - a strip cannot know the
    middle row of the raster; DinfAvalanche gets row0 / ny_total and the whole raster's geometry.  Returns the owned rows as numpy arrays."""
    import torch

    from taudem_amd.distributed import strip_rows

    ang, p = put(inp["ang"]), put(inp["p"])
    out = {}
    out["qrl"], _ = pipe.retlimflow(ang, put(inp["wg"]), put(inp["rc"]), dx=sdx, dy=sdy)
    out["zfdc"], _ = pipe.flowdircond(p, put(inp["z"]), z_nodata=FEL_ND)
    out["vd"], _ = pipe.d8vdisttostrm(p, put(inp["feld"]), put(inp["src32"]), 1, src_nodata=SRC_ND)    # (fel's halo rows are written by the call)
    out["vd_none"], _ = pipe.d8vdisttostrm(p, put(inp["feld"]), put(inp["src32_none"]), 1, src_nodata=SRC_ND)
    out["vd_ad8"], _ = pipe.d8vdisttostrm(p, put(inp["feld"]), put(inp["ad8i"]), 40, src_nodata=SRC_ND)
    for k, dn, niter in niter_of_whole:
        out[k], _ = pipe.slopeavedown(p, put(inp["feld"]), dn, niter, dx=sdx, dy=sdy, fel_nodata=FEL_ND)
    adx, ady = (strip_rows(a, y0, y1) for a in inp["aval_cells"])
    feld, ang_a = put(inp["feld"]), put(inp["ang_a"])
    for sfx, d, ta, ass in _aval_inputs(inp):
        out["rz" + sfx], out["dfs" + sfx], _ = pipe.dinfavalanche(ang_a, feld, put(ass), row0=y0, ny_total=ny_total, thresh=ta[0], alpha=ta[1], direct=d,
                                                                  dx=adx, dy=ady, geo=inp["aval_geo"])
    torch.cuda.synchronize()
    return {k: v[1:y1 - y0 + 1].cpu().numpy() for k, v in out.items()}


def compare_late(got, ref, what):
    """qrl, zfdc, vd* and slpd* bit for bit; rz / dfs by aval_model.compare_aval, which prints the cells with rz data and the tainted share
    of every run.  Returns the list of failures."""
    from conftest import bits_equal, describe_diff

    want = [k for k in ref if not k.startswith("taint")]
    bad = [f"{what}: {k} not computed" for k in want if k not in got]
    for k in LATE_BITWISE:
        if k in got and not bits_equal(np.asarray(got[k]), ref[k]):
            bad.append(describe_diff(np.asarray(got[k]), ref[k], f"{what}: {k}"))
    for sfx, _, _ in aval_runs():
        if "rz" + sfx in got and "rz" + sfx in ref:
            bad += aval_model.compare_aval(np.ascontiguousarray(got["rz" + sfx]), np.ascontiguousarray(got["dfs" + sfx]), ref["rz" + sfx], ref["dfs" + sfx],
                                           ref["taint" + sfx], f"{what}: rz{sfx} / dfs{sfx}")
    return bad
