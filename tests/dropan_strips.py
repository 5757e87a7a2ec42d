"""DropAnalysis in row strips: the helpers of tests/test_gpu_dropan.py, tests/test_gpu_dropan_strips.py, tests/test_gpu_dropan_pathological.py and
tests/test_dropan_strips_model.py.  A helper module, not a conftest.

    outlets(p, ad8)             the outlets the tests use: the largest-area cells, one twice, one off the raster
    cut_outlets(p, ad8, parts)  ... and the largest-area cell with a direction on both rows of every cut
    check(ctx, restate, ...)    the one-device form against the restatement (tests/dropan_model.py)
    near(got, want, noise)      two tables of two summation orders
    in_strips(...)              StripPipeline.dropanalysis on any list of row ranges, one rank per range: the strips' results and their combination
    combine(results, ...)       what a caller of the strip form does with the strips' results
    expected_split(...)         what every strip must report, from the restatement's order / elevOut grids, in numpy
    assert_strips(...)          the assertions on a combination and on every strip's own numbers; it takes arrays, no context

What is exact and what is not is said in tests/test_gpu_dropan.py.  Adding the strips' fp64 partial sums in strip order is still one summation tree over the
same n terms, so the bound gamma_n * sum|x| of the one-device form holds for the combination unchanged; the length takes one more rounding per strip.
A strip's own counts are derived here, not taken from the restatement's totals: a junction is a cell with a record and at least two inflows with a record,
each inflow of lower order than the junction's is one drop (first-order if the inflow's order is 1), and the strip that owns the junction's row counts it.
Where a sum is NaN or infinite (rasters with NaN / Inf cells) the comparison is by class: NaN, +Inf, -Inf or finite, the same in the same place.
"""
import math

import numpy as np

import dropan_model as M
from conftest import bits_equal, describe_diff

DX = (0, 1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, 0, -1, -1, -1, 0, 1, 1, 1)
HALO_FILL = 12345.0            # neither data of any test raster nor a nodata value
HALO_P = (7, 3)                # halo rows of p before the call: the row above points south, the row below north - into the owned rows


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------
def outlets(p, ad8, n=3):
    """the n largest-area cells that have a direction, one cell twice and one off the raster"""
    ny, nx = p.shape
    a = np.where((p >= 1) & (p <= 8), ad8, -2.0).ravel()
    idx = np.argsort(-a, kind="stable")[:n]
    idx = idx[a[idx] > -2.0]
    cols, rows = list(idx % nx) + [nx + 3], list(idx // nx) + [0]
    if len(idx):
        cols.append(cols[0])
        rows.append(rows[0])
    return np.array(cols, np.int32), np.array(rows, np.int32)


def cut_outlets(p, ad8, parts, n=3):
    """outlets() and, for every cut, the largest-ad8 cell with a direction on the rows y0 - 1 and y0 (a row without one adds nothing)"""
    cols, rows = (list(v) for v in outlets(p, ad8, n))
    for y0, _ in parts[1:]:
        for y in (y0 - 1, y0):
            a = np.where((p[y] >= 1) & (p[y] <= 8), ad8[y], -2.0)
            x = int(np.argmax(a))
            if a[x] > -2.0:
                cols.append(x)
                rows.append(y)
    return np.array(cols, np.int32), np.array(rows, np.int32)


SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
ONE_ROW_SEED, EDGE_SEED = 2, 5     # a strip of exactly one owned row; cuts directly under row 0 and directly above the last row
NTHRESH = 6


def ladder_of(ssa, steptype):
    """(tmin, tmax, nthresh) of a random case: a log ladder up to a quarter of the largest ssa, an arithmetic one over the first few tens of cells"""
    return (2.0, float(ssa.max()) / 4.0, NTHRESH) if steptype == 0 else (2.0, 27.0, NTHRESH)


def random_case(oracle, peuker, seed):
    """One case of the random cuts: a fractal of about 200 x 300 with 10 nodata blocks, 2 to 6 strips cut at random distinct rows, the cell sizes, the
    eager-round switch, the grid threshold and the ssa rotating with the seed.  fel, p, ad8 are the CPU oracle's; every second seed takes as ssa
    the oracle's aread8 weighted with the Peuker-Douglas grid of tests/peuker_model.py (`peuker`: its compiled restatement)."""
    from cellsizes import rows as cell_rows

    rng = np.random.default_rng(900 + seed)
    ny, nx = 200 + int(rng.integers(0, 9)), 300 + int(rng.integers(0, 9))
    z = oracle.synth_dem((ny, nx), 500 + seed)
    for _ in range(10):
        y, x = int(rng.integers(0, ny)), int(rng.integers(0, nx))
        z[max(y - 3, 0):y + 4, max(x - 5, 0):x + 6] = -9999.0
    world = int(rng.integers(2, 7))
    cuts = sorted(rng.choice(np.arange(1, ny), world - 1, replace=False).tolist())
    if seed == ONE_ROW_SEED:
        cuts = sorted(set(cuts) | {cuts[0] + 1})
    if seed == EDGE_SEED:
        cuts = sorted(set(cuts) | {1, ny - 1})
    parts = list(zip([0] + cuts, cuts + [ny]))
    dx, dy = [(30.0, 25.0), cell_rows("wild", ny, seed), cell_rows("band", ny)][seed % 3]
    fel = oracle.pitremove(z, -9999.0)
    p, _, _ = oracle.d8flowdir(fel, -3.0e38, dx, dy)
    ad8 = oracle.aread8(p, -32768, contcheck=False)
    ssa = ad8
    if seed % 2:
        ssa = oracle.aread8(p, -32768, weights=peuker.run(fel).astype(np.float32), contcheck=False)
    cols, rows = cut_outlets(p, ad8, parts)
    return {"ny": ny, "nx": nx, "parts": parts, "dx": dx, "dy": dy, "fel": fel, "p": p, "ad8": ad8, "ssa": ssa, "cols": cols, "rows": rows,
            "eager": (1, 2, 8)[(seed + seed // 3) % 3], "grid_th": seed % NTHRESH}


def patho_case(oracle, name):
    """fel, p, ad8 of the raster `name` of tests/pathological.py through the CPU oracle (30 x 30 cells), the outlets of outlets() and a log ladder of five
    thresholds from 2 to a quarter of the largest area (of 8 where no area reaches it); ssa = ad8"""
    import pathological as PG

    dem = np.ascontiguousarray(PG.CASES[name](oracle), np.float32)
    fel = oracle.pitremove(dem, PG.NODATA)
    p, _, _ = oracle.d8flowdir(fel, -3.0e38, 30.0, 30.0)
    ad8 = oracle.aread8(p, -32768, contcheck=False)
    cols, rows = outlets(p, ad8)
    return {"fel": fel, "p": p, "ad8": ad8, "cols": cols, "rows": rows, "dx": 30.0, "dy": 30.0, "par": (2.0, max(8.0, float(ad8.max())) / 4.0, 5)}


def input_conditions(ref, p, parts):
    """(written rows, n2 of the first written row, min ||t| - 2| over the console lines, junctions on cut rows at the lowest threshold): what the random
    cuts ask of their inputs, from the restatement alone"""
    rows, _ = M.parse_table(ref["table"])
    ts = M.console_t(ref["console"])
    return len(rows), int(rows[0, 3]) if len(rows) else 0, float(np.min(np.abs(np.abs(ts) - 2.0))) if ts.size else math.inf, junctions_on_cut_rows(ref["per"][0]["order"], p, parts)


# ---- sums that may be NaN or infinite ---------------------------------------------------------------------------------------------------------------
def value_class(v):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf"""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), 1, np.where(np.isposinf(v), 2, np.where(np.isneginf(v), 3, 0)))


def _fsum(x):
    """math.fsum; where a term is NaN or infinite, the value every summation order gives (NaN, or the infinity of the only sign present)"""
    x = np.asarray(x, np.float64)
    if np.all(np.isfinite(x)):
        return math.fsum(x)
    if np.isnan(x).any() or (np.isposinf(x).any() and np.isneginf(x).any()):
        return math.nan
    return math.inf if np.isposinf(x).any() else -math.inf


def _sq(d):
    with np.errstate(over="ignore", invalid="ignore"):
        return (d * d).astype(np.float32)     # the float square, as the reference forms it


def exact_sums(d1, d2):
    """M.sums_from_drops that also takes drops that are NaN or infinite"""
    return [_fsum(d1), _fsum(_sq(d1)), _fsum(d2), _fsum(_sq(d2))]


def abs_sums(d1, d2):
    return [_fsum(np.abs(d1)), _fsum(_sq(d1)), _fsum(np.abs(d2)), _fsum(_sq(d2))]


def sum_within(got, exact, mag, nterms):
    """|got - exact| <= gamma_n * sum|x| for a finite exact sum; the same class of value otherwise"""
    if math.isfinite(exact) and math.isfinite(mag):
        return abs(float(got) - exact) <= M.gamma(max(nterms, 1)) * mag
    return int(value_class(got)) == int(value_class(exact))


def same_tables(got, want, nan_aware=False):
    """the rows that are written, their counts and the optimum; with nan_aware also the class of every other column"""
    a, oa = M.parse_table(got)
    b, ob = M.parse_table(want)
    if a.shape != b.shape or not np.array_equal(a[:, [0, 2, 3]], b[:, [0, 2, 3]]) or oa != ob:
        return False
    return not nan_aware or bool(np.array_equal(value_class(a), value_class(b)))


# ---- one device -------------------------------------------------------------------------------------------------------------------------------------
def check(ctx, restate, ad8, p, fel, ssa, cols, rows, dx, dy, par, st, what, grid_th=1, ssa_nodata=-1.0, nan_aware=False):
    """One run against the restatement: everything exact but the four sums and the length, which are held to the fp64 bounds of tests/test_gpu_dropan.py."""
    ny, nx = p.shape
    dxc, dyc = M._f64(dx, ny), M._f64(dy, ny)
    thresh, n1, n2, sums, length, area, table, opt, order, elev = ctx.dropanalysis(ad8, p, fel, ssa, (cols, rows), thresh_min=par[0], thresh_max=par[1], nthresh=par[2],
                                                                                   steptype=st, dx=dx, dy=dy, ssa_nodata=ssa_nodata, grids=grid_th)
    ref = restate.run(ad8, p, fel, ssa, cols, rows, dxc, dyc, par[0], par[1], par[2], st, ssa_nodata=ssa_nodata)
    assert bits_equal(thresh, ref["thresh"]), f"{what}: ladder"
    assert bits_equal(np.float32(area).reshape(1), np.float32(ref["total_area"]).reshape(1)), f"{what}: total area {area} vs {ref['total_area']}"
    for th, q in enumerate(ref["per"]):
        assert (int(n1[th]), int(n2[th])) == (q["n1"], q["n2"]), f"{what}: n1, n2 of threshold {th}"
        exact, mag = exact_sums(q["drops1"], q["drops2"]), abs_sums(q["drops1"], q["drops2"])
        for k, nterms in enumerate((q["n1"], q["n1"], q["n2"], q["n2"])):
            assert sum_within(sums[th, k], exact[k], mag[k], nterms), f"{what}: sum {k} of threshold {th}: {sums[th, k]!r} vs {exact[k]!r}"
        want_len, links = M.exact_length(q["order"], p, dxc, dyc)
        assert abs(float(length[th]) - want_len) <= M.gamma(links + 3 * ny) * want_len, f"{what}: length of threshold {th}: {length[th]!r} vs {want_len!r}"
    q = ref["per"][grid_th]
    assert bits_equal(order, q["order"]), describe_diff(order, q["order"], f"{what}: order grid")
    assert bits_equal(elev, q["elev"]), describe_diff(elev, q["elev"], f"{what}: elevOut grid")
    # the table from our sums: the rows that appear and the optimum are the restatement's wherever no |t| is near 2
    got, _ = M.parse_table(table.encode())
    want, _ = M.parse_table(ref["table"])
    assert np.array_equal(got[:, [0, 2, 3]], want[:, [0, 2, 3]]), f"{what}: rows of the table"
    if nan_aware:
        assert np.array_equal(value_class(got), value_class(want)), f"{what}: classes of the table's values\n{table}\n{ref['table'].decode()}"
    return ref, (thresh, n1, n2, sums, length, area, table, opt)


def near(got, want, noise):
    """Tables of two summation orders (the strips add their fp64 sums in strip order): the same rows and optimum, and the printed values as close as the
    golden test asks of two summation orders - DrainDen 2e-6 relative, the other columns 2 * noise + 2e-6 (2e-6: one unit of the %f print on each side)."""
    a, oa = M.parse_table(got)
    b, ob = M.parse_table(want)
    return (oa == ob and a.shape == b.shape and np.array_equal(a[:, [0, 2, 3]], b[:, [0, 2, 3]]) and bool(np.all(np.abs(a[:, 1] - b[:, 1]) <= 2e-6 * np.abs(b[:, 1])))
            and bool(np.all(np.abs(a[:, 4:] - b[:, 4:]) <= 2.0 * noise + 2e-6)))


# ---- strips on the device -----------------------------------------------------------------------------------------------------------------------------
def in_strips(z_inputs, parts, dx, dy, outlets, par, steptype, grid_th, ssa_nodata=-1.0):  # noqa: A002
    """StripPipeline.dropanalysis on z_inputs = (ad8, p, fel, ssa) cut into the row ranges parts = [(y0, y1)], each on a rank of its own.  The halo rows hold
    values that are neither data nor nodata before the call (p: directions that point into the owned rows); each strip gets its own rows of the
    global per-row dx / dy through strip_rows and its outlets through local_outlets.  Returns (results, combined): the strips' results as the
    call gave them (the two grids as host arrays of the strip array's shape, the stats dict last) and combine() of them."""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline, strip_rows

    ad8, p, fel, ssa = z_inputs
    nx = p.shape[1]
    cols, rows = outlets
    with StripGroup(len(parts), nx, [0] * len(parts)) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            nyl = y1 - y0
            pipe = StripPipeline(c, comm, nx, nyl)

            def put(a):
                t = pipe.empty(getattr(torch, np.asarray(a).dtype.name))
                if a.dtype == np.int16:
                    t[0].fill_(HALO_P[0])
                    t[nyl + 1].fill_(HALO_P[1])
                else:
                    t[0].fill_(HALO_FILL)
                    t[nyl + 1].fill_(HALO_FILL)
                t[1:nyl + 1] = torch.from_numpy(np.ascontiguousarray(a[y0:y1])).cuda()
                return t
            t_ad8, t_p, t_fel = put(ad8), put(p), put(fel)
            t_ssa = t_ad8.clone() if ssa is ad8 else put(ssa)
            res = pipe.dropanalysis(t_ad8, t_p, t_fel, t_ssa, pipe.local_outlets(cols, rows, y0), par[0], par[1], par[2], steptype, strip_rows(dx, y0, y1),
                                    strip_rows(dy, y0, y1), ssa_nodata=ssa_nodata, grids=grid_th)
            torch.cuda.synchronize()
            return res[:6] + (res[6].cpu().numpy(), res[7].cpu().numpy()) + res[8:]
        results = grp.run(rank_main)
    return results, combine(results, parts, dx, dy)


def combine(results, parts, dx, dy):
    """What the caller of the strip form does: n1 / n2 added, the fp64 sums and lengths added IN STRIP ORDER, the outlets' terms added in file order as
    float32 and multiplied with the cell area of the raster's middle row, the owned rows of the two grids concatenated.  results[r] = (thresh, n1, n2,
    sums, length, outlet_term, order, elevOut, ...) of the strip parts[r], the grids as strip arrays (a halo row on each side)."""
    ny = parts[-1][1]
    dxc, dyc = M._f64(dx, ny), M._f64(dy, ny)
    n1, n2 = np.zeros_like(results[0][1]), np.zeros_like(results[0][2])
    sums, length = np.zeros_like(results[0][3]), np.zeros_like(results[0][4])
    term = np.zeros_like(results[0][5])
    for r in results:                                  # strip order
        n1, n2 = n1 + r[1], n2 + r[2]
        sums, length = sums + r[3], length + r[4]
        term = (term + r[5]).astype(np.float32)        # one strip owns an outlet, the others say 0
    ta = np.float32(0.0)
    for t in term:                                     # file order
        ta = np.float32(ta + t)
    with np.errstate(over="ignore", invalid="ignore"):
        area = np.float32(float(ta) * abs(dxc[ny // 2]) * abs(dyc[ny // 2]))
    own = lambda k: np.concatenate([r[k][1:-1] for r in results], axis=0)  # noqa: E731  (a strip array without its two halo rows)
    return {"thresh": results[0][0], "thresh_all": [r[0] for r in results], "n1": n1, "n2": n2, "sums": sums, "length": length, "area": area, "order": own(6), "elev": own(7)}


# ---- what every strip must report, in numpy ---------------------------------------------------------------------------------------------------------------
def _inflows(order, p):
    """(has, count, [(k, mask, y of the inflow, x of the inflow)]): for every neighbour k, the cells whose neighbour k has a record and points at them"""
    ny, nx = order.shape
    has = order != M.ORDER_NODATA
    count = np.zeros((ny, nx), np.int32)
    per_k = []
    yy, xx = np.mgrid[0:ny, 0:nx]
    for k in range(1, 9):
        yn, xn = yy + DY[k], xx + DX[k]
        ok = (yn >= 0) & (yn < ny) & (xn >= 0) & (xn < nx)
        ync, xnc = np.clip(yn, 0, ny - 1), np.clip(xn, 0, nx - 1)
        m = ok & has[ync, xnc] & (p[ync, xnc] == (k + 3) % 8 + 1)       # the direction opposite to k points back at the cell
        count += m
        per_k.append((k, m, ync, xnc))
    return has, count, per_k


def junction_drops(order, elev, p, fel):
    """(jy, jx, inflow's order, drop): one entry per drop - per inflow of lower order of every junction, the junctions in row-major order and their inflows
    in neighbour order; drop = elevOut of the inflow - fel of the junction, in float.  Also returns the junction mask."""
    has, count, per_k = _inflows(order, p)
    junction = has & (count >= 2)
    jy, jx, jo, jd, jk = [], [], [], [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for k, m, yn, xn in per_k:
            sel = junction & m & (order[yn, xn] < order)
            ys, xs = np.nonzero(sel)
            jy.append(ys); jx.append(xs); jo.append(order[yn[ys, xs], xn[ys, xs]])
            jd.append((elev[yn[ys, xs], xn[ys, xs]] - fel[ys, xs]).astype(np.float32))
            jk.append(np.full(ys.size, k))
    jy, jx, jo, jd, jk = (np.concatenate(v) for v in (jy, jx, jo, jd, jk))
    o = np.lexsort((jk, jx, jy))
    return (jy[o], jx[o], jo[o], jd[o]), junction


def junctions_on_cut_rows(order, p, parts):
    """the number of junctions on the rows next to a cut: the last owned row of the strip above it and the first owned row of the strip below"""
    has, count, _ = _inflows(order, p)
    junction = has & (count >= 2)
    return int(junction[sorted({y for y0, _ in parts[1:] for y in (y0 - 1, y0)})].sum())


def _strip_length(order, p, sdx, sdy, y0, y1):
    """(length, links) of the links whose RECEIVING cell lies in the rows [y0, y1), measured with the strip array's rows sdx / sdy (row y of the raster is row
    y - y0 + 1 of the strip array); a scalar cell size serves every row"""
    has, _, per_k = _inflows(order, p)
    terms = []
    for k, m, _, _ in per_k:
        ys = np.nonzero((m & has)[y0:y1])[0] + 1
        ex, ey = (np.broadcast_to(np.asarray(v, np.float64), (y1 - y0 + 2,))[ys] for v in (sdx, sdy))
        terms.append(ex if k in (1, 5) else ey if k in (3, 7) else np.sqrt(ex * ex + ey * ey))
    t = np.concatenate(terms)
    return math.fsum(t), int(t.size)


def expected_split(ref, p, fel, ad8, ssa, outlets, parts, dx, dy, grid_th, ssa_nodata=-1.0, shift_rows=0):  # noqa: A002
    """The restatement's own per-strip split, in the layout of the strip form's results: per strip (thresh, n1, n2, sums, length, outlet_term, order, elevOut)
    with the two grids as strip arrays.  The sums are math.fsum of the strip's drops, the length that of the strip's links with the strip's rows of
    strip_rows(dx / dy, y0 + shift_rows, y1 + shift_rows) - shift_rows != 0 is the one-row shift the sensitivity test plants."""
    from taudem_amd.distributed import strip_rows

    ny, nx = p.shape
    nt = len(ref["thresh"])
    cols, rows = outlets
    out = []
    drops = [junction_drops(q["order"], q["elev"], p, fel)[0] for q in ref["per"]]
    for y0, y1 in parts:
        n1, n2, sums, length = np.zeros(nt, np.int64), np.zeros(nt, np.int64), np.zeros((nt, 4), np.float64), np.zeros(nt, np.float64)
        sdx, sdy = strip_rows(dx, y0, y1), strip_rows(dy, y0, y1)
        if shift_rows:
            shifted = np.clip(np.arange(y0 - 1, y1 + 1) + shift_rows, 0, ny - 1)
            sdx, sdy = M._f64(dx, ny)[shifted], M._f64(dy, ny)[shifted]
        for th, q in enumerate(ref["per"]):
            jy, _, jo, jd = drops[th]
            mine = (jy >= y0) & (jy < y1)
            d1, d2 = jd[mine & (jo == 1)], jd[mine & (jo != 1)]
            n1[th], n2[th] = d1.size, d2.size
            sums[th] = exact_sums(d1, d2)
            length[th] = _strip_length(q["order"], p, sdx, sdy, y0, y1)[0]
        term = np.zeros(len(cols), np.float32)
        for i, (x, y) in enumerate(zip(cols.tolist(), rows.tolist())):
            if 0 <= x < nx and y0 <= y < y1:
                d = int(p[y, x])
                xn, yn = x + DX[d], y + DY[d]
                inside = 0 <= xn < nx and 0 <= yn < ny
                if not inside or abs(np.float32(ssa[yn, xn]) - np.float32(ssa_nodata)) < 1e-5 or ssa[yn, xn] <= 0:
                    term[i] = ad8[y, x]
        q = ref["per"][grid_th]
        grid = lambda a, fill: np.concatenate([np.full((1, nx), fill, a.dtype), a[y0:y1], np.full((1, nx), fill, a.dtype)], axis=0)  # noqa: E731
        out.append((ref["thresh"].copy(), n1, n2, sums, length, term, grid(q["order"], M.ORDER_NODATA), grid(q["elev"], M.ELEV_NODATA)))
    return out


# ---- the assertions -----------------------------------------------------------------------------------------------------------------------------------
def assert_strips(results, comb, ref, p, fel, parts, dx, dy, grid_th, what, nan_aware=False):
    """The combination of the strips against the restatement of the WHOLE raster with the global per-row sizes, and every strip's own counts and sums against
    the split derived from the restatement's grids.  Takes arrays only: results / comb as in_strips returns them (or expected_split and combine)."""
    import taudem_amd as T

    ny = p.shape[0]
    nstrips = len(parts)
    dxc, dyc = M._f64(dx, ny), M._f64(dy, ny)
    assert len(results) == nstrips and parts[0][0] == 0 and parts[-1][1] == ny and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
    for r, t in enumerate(comb["thresh_all"]):
        assert bits_equal(t, ref["thresh"]), f"{what}: ladder of strip {r}"
    assert bits_equal(np.float32(comb["area"]).reshape(1), np.float32(ref["total_area"]).reshape(1)), f"{what}: total area {comb['area']} vs {ref['total_area']}"
    for th, q in enumerate(ref["per"]):
        assert (int(comb["n1"][th]), int(comb["n2"][th])) == (q["n1"], q["n2"]), f"{what}: n1, n2 of threshold {th}: {comb['n1'][th]}, {comb['n2'][th]} vs {q['n1']}, {q['n2']}"
        exact, mag = exact_sums(q["drops1"], q["drops2"]), abs_sums(q["drops1"], q["drops2"])
        for k, nterms in enumerate((q["n1"], q["n1"], q["n2"], q["n2"])):
            assert sum_within(comb["sums"][th, k], exact[k], mag[k], nterms), f"{what}: sum {k} of threshold {th}: {comb['sums'][th, k]!r} vs {exact[k]!r}"
        want_len, links = M.exact_length(q["order"], p, dxc, dyc)
        assert abs(float(comb["length"][th]) - want_len) <= M.gamma(links + 3 * ny + nstrips) * want_len, f"{what}: length of threshold {th}: {comb['length'][th]!r} vs {want_len!r}"
        # every strip's own numbers: a drop counted twice in one strip and dropped in another must not cancel out
        (jy, _, jo, jd), _ = junction_drops(q["order"], q["elev"], p, fel)
        assert (int(np.sum(jo == 1)), int(np.sum(jo != 1))) == (q["n1"], q["n2"]), f"{what}: the drops derived from the grids are not the restatement's (threshold {th})"
        for r, (y0, y1) in enumerate(parts):
            mine = (jy >= y0) & (jy < y1)
            d1, d2 = jd[mine & (jo == 1)], jd[mine & (jo != 1)]
            got = (int(results[r][1][th]), int(results[r][2][th]))
            assert got == (d1.size, d2.size), f"{what}: strip {r} (rows {y0}..{y1 - 1}), threshold {th}: n1, n2 = {got}, its junctions have {(d1.size, d2.size)}"
            exact_r, mag_r = exact_sums(d1, d2), abs_sums(d1, d2)
            for k, nterms in enumerate((d1.size, d1.size, d2.size, d2.size)):
                assert sum_within(results[r][3][th, k], exact_r[k], mag_r[k], nterms), f"{what}: strip {r}, threshold {th}, sum {k}: {results[r][3][th, k]!r} vs {exact_r[k]!r}"
    q = ref["per"][grid_th]
    assert comb["order"].shape == q["order"].shape and comb["elev"].shape == q["elev"].shape, f"{what}: the strips' owned rows do not make the raster"
    assert all(r[6].shape[0] == y1 - y0 + 2 for r, (y0, y1) in zip(results, parts)), f"{what}: order grid: a strip's array has other rows than the strip"
    assert bits_equal(comb["order"], q["order"]), describe_diff(comb["order"], q["order"], f"{what}: order grid")
    assert bits_equal(comb["elev"], q["elev"]), describe_diff(comb["elev"], q["elev"], f"{what}: elevOut grid")
    # the table of the combined values: the written rows and the optimum are the restatement's (no |t| of the inputs is near 2)
    with np.errstate(over="ignore", invalid="ignore"):
        s = comb["sums"].astype(np.float32)
    table, _, opt = T.dropanalysis_table(comb["thresh"], comb["n1"], comb["n2"], s[:, 0], s[:, 1], s[:, 2], s[:, 3], comb["length"], comb["area"])
    assert same_tables(table.encode(), ref["table"], nan_aware), f"{what}: table\n{table}\n{ref['table'].decode()}"
    assert (opt is None) == (ref["optimum"] is None) and (opt is None or np.float32(opt) == ref["optimum"]), f"{what}: optimum {opt} vs {ref['optimum']}"
    return table
