"""PeukerDouglas on the GPU (taudem_amd/csrc/peuker.hip) against the reference's rasters (tests/golden/peuker_*.npz) where there is one, and against the
serial restatement elsewhere (tests/peuker_model.py, held to those rasters by tests/test_peuker_restatement.py).  The output is 0 / 1: every comparison is
np.array_equal, there is no tolerance anywhere.  The restatement scans the 2x2 groups one after the other and clears flags as it goes; the kernels
take the union of what the groups clear, per cell: the two formulations check each other."""
import os
import subprocess

import numpy as np
import pytest

import dropan_model as DM
import peuker_model as M
import taudem_amd as T
from taudem_amd import _lib, tools

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")
# mirrors of PK_SEG and PK_COLS in taudem_amd/csrc/peuker.hip: rows per lane segment, output columns per wave.  A block is four waves that are four
# segments of the SAME columns, so the output columns per block are those of a wave and a block ends every 4 * SEG rows.  One instantiation.
SEG, WAVE_COLS, BLOCK_COLS, BLOCK_ROWS = 32, 60, 60, 4 * 32
NYS = sorted({1, 2, 3, 4, 5, SEG - 1, SEG, SEG + 1, 2 * SEG + 1, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1})
NXS = sorted({1, 2, 3, 4, 5, WAVE_COLS - 1, WAVE_COLS, WAVE_COLS + 1, 2 * WAVE_COLS - 1, 2 * WAVE_COLS, 2 * WAVE_COLS + 1, BLOCK_COLS + 1})
NODATA = np.float32(-9999.0)


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("peuker"))


@pytest.fixture(scope="module")
def base(oracle):
    """the seeded fractal every seam shape is a crop of"""
    return oracle.synth_dem((max(NYS), max(NXS)), 4242)


def _dev(ctx, z, nodata, weights=M.DEFAULT, **kw):
    import torch

    out = ctx.peukerdouglas(torch.from_numpy(np.ascontiguousarray(z)).cuda(), float(nodata), weights, **kw)
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()


def _twopass(ctx, z, nodata, weights=M.DEFAULT, float_weights=False):
    """the two kernels with the smoothed grid in scratch between them: the strip form on a single strip, comm == NULL.  The halo rows hold
    something that is neither data of the raster nor nodata: the library fills them."""
    import torch

    from taudem_amd.distributed import StripPipeline

    ny, nx = z.shape
    pipe = StripPipeline(ctx, None, nx, ny)
    t = pipe.empty(torch.float32)
    t.fill_(12345.0)
    t[1:ny + 1] = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    out = pipe.peukerdouglas(t, float(nodata), weights, float_weights)
    return tuple(o[1:ny + 1].cpu().numpy() for o in out[:-1]) if float_weights else out[0][1:ny + 1].cpu().numpy()


def _punched(z):
    """nodata holes on the kernel's seams: one across a wave boundary (columns 58..62), one across a segment boundary (rows 30..34), one on the
    crossing of the two and one across the block's last row; what lies outside the crop is clipped.  A crop too small for any gets one cell."""
    z = z.copy()
    z[2:6, WAVE_COLS - 2:WAVE_COLS + 3] = NODATA
    z[SEG - 2:SEG + 3, 3:8] = NODATA
    z[SEG - 1:SEG + 1, WAVE_COLS - 1:WAVE_COLS + 1] = NODATA
    z[BLOCK_ROWS - 1:BLOCK_ROWS + 1, 2 * WAVE_COLS - 3:2 * WAVE_COLS + 2] = NODATA
    if not (z == NODATA).any():
        z[z.shape[0] // 2, z.shape[1] // 2] = NODATA
    return z


# ---- goldens --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES)
def test_cases_against_the_reference(ctx, case):
    gold = M.load_golden(case)
    for key, z, nd, w in M.golden_runs(case):
        host = ctx.peukerdouglas(z, float(nd), w)
        assert host.dtype == np.int16 and np.array_equal(host, gold[key]), (case, key, "host form", int(np.sum(host != gold[key])))
        dev = _dev(ctx, z, nd, w)
        assert dev.dtype == np.int16 and np.array_equal(dev, gold[key]), (case, key, "device form", int(np.sum(dev != gold[key])))


def test_pathological_rasters_against_the_reference(ctx):
    gold = M.load_golden("patho")
    for name, z in M.patho_inputs():
        host, dev = ctx.peukerdouglas(z, -9999.0), _dev(ctx, z, -9999.0)
        assert np.array_equal(host, gold[name]), (name, "host form", int(np.sum(host != gold[name])))
        assert np.array_equal(dev, gold[name]), (name, "device form", int(np.sum(dev != gold[name])))


# ---- shapes at the kernel's seams -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny", NYS)
def test_seam_shapes_fused_and_two_pass(ctx, restate, base, ny):
    """every crop (ny, nx), plain and with holes on the seams: the fused kernel, with and without the float copy, and the two-kernel path, all
    equal to the restatement"""
    flagged = 0
    for nx in NXS:
        for holes in (False, True):
            z = np.ascontiguousarray(base[:ny, :nx])
            z = _punched(z) if holes else z
            want = restate.run(z, NODATA)
            what = (ny, nx, "holes" if holes else "plain")
            ss = _dev(ctx, z, NODATA)
            assert np.array_equal(ss, want), (*what, "fused", np.argwhere(ss != want)[:5].tolist())
            ss2, w = _dev(ctx, z, NODATA, float_weights=True)
            assert np.array_equal(ss2, ss) and w.dtype == np.float32 and np.array_equal(w, ss.astype(np.float32)), (*what, "float weights")
            two = _twopass(ctx, z, NODATA)
            assert np.array_equal(two, ss), (*what, "two-pass", np.argwhere(two != ss)[:5].tolist())
            flagged += int(want.sum())
    assert ny < 3 or flagged > 0


def test_two_pass_float_weights_and_other_weights(ctx, restate, base):
    z = _punched(base[:SEG + 1, :2 * WAVE_COLS + 1])
    for w in M.PARS:
        want = restate.run(z, NODATA, w)
        ss, wf = _twopass(ctx, z, NODATA, w, float_weights=True)
        assert np.array_equal(ss, want) and np.array_equal(wf, want.astype(np.float32)), w
        assert np.array_equal(_dev(ctx, z, NODATA, w), want), w


def test_two_pass_switch_of_the_device_form(ctx, restate, base, monkeypatch):
    z = _punched(base[:2 * SEG + 1, :2 * WAVE_COLS + 1])
    want = restate.run(z, NODATA)
    _, st = ctx.peukerdouglas(z, float(NODATA), stats=True)
    assert st["launches_stencil"] == 1
    monkeypatch.setenv("TDX_PEUKER_TWOPASS", "1")
    ss, st = ctx.peukerdouglas(z, float(NODATA), stats=True)
    assert np.array_equal(ss, want) and st["launches_stencil"] == 2


def test_out_arguments_and_refusals(ctx, base):
    import torch

    z = np.ascontiguousarray(base[:40, :70])
    ss, w = np.zeros(z.shape, np.int16), np.zeros(z.shape, np.float32)
    r = ctx.peukerdouglas(z, float(NODATA), float_weights=True, out=(ss, w))
    assert r[0] is ss and r[1] is w and ss.any() and np.array_equal(w, ss.astype(np.float32))
    zt = torch.from_numpy(z).cuda()
    for bad in (z.astype(np.float64), z[:, ::2], z.T):
        with pytest.raises(ValueError):
            ctx.peukerdouglas(bad)
    with pytest.raises(ValueError):
        ctx.peukerdouglas(z, out=np.zeros((3, 3), np.int16))
    with pytest.raises(ValueError):
        ctx.peukerdouglas(zt, out=np.zeros(z.shape, np.int16))   # a host output for a device input
    with pytest.raises(ValueError):
        ctx.peukerdouglas(z, weights=(0.4, 0.1))


# ---- strips -----------------------------------------------------------------------------------------------------------------------------------
def _in_strips(z, nodata, parts, weights=M.DEFAULT):
    """ss of z cut into the row strips `parts` ([(y0, y1)]), each strip through tdx_peukerdouglas_strip on a rank of its own: the owned rows, concatenated"""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline

    nx = z.shape[1]
    with StripGroup(len(parts), nx, [0] * len(parts)) as grp:
        def rank_main(r, c, comm):
            y0, y1 = parts[r]
            pipe = StripPipeline(c, comm, nx, y1 - y0)
            t = pipe.empty(torch.float32)
            t.fill_(12345.0)
            t[1:y1 - y0 + 1] = torch.from_numpy(np.ascontiguousarray(z[y0:y1])).cuda()
            ss, w, _ = pipe.peukerdouglas(t, float(nodata), weights, True)
            return ss[1:y1 - y0 + 1].cpu().numpy(), w[1:y1 - y0 + 1].cpu().numpy()
        res = grp.run(rank_main)
    return np.concatenate([r[0] for r in res], axis=0), np.concatenate([r[1] for r in res], axis=0)


def _strip_rasters(base):
    from taudem_amd.distributed import partition_rows

    g = np.load(os.path.join(M.GOLDEN, "case_holes.npz"))
    wide7, wide3 = base[:7, :70].copy(), base[:3, :70].copy()
    wide7[0:3, 20:24] = NODATA   # a hole through the cut under row 0 and the next one
    wide7[5:7, 40:45] = NODATA   # ... and through the cut above the last row
    wide3[1, 30:33] = NODATA
    out = [(f"holes in {n}", g["fel"], M.FEL_NODATA, partition_rows(g["fel"].shape[0], n)) for n in (2, 3, 5)]
    # 7 rows: the cut directly under row 0, the cut directly above the last row, strips of ONE owned row in between
    out += [("7x70 in 2", wide7, NODATA, [(0, 1), (1, 7)]), ("7x70 in 3", wide7, NODATA, [(0, 3), (3, 6), (6, 7)]),
            ("7x70 in 5", wide7, NODATA, [(0, 1), (1, 2), (2, 4), (4, 6), (6, 7)])]
    # 3 rows hold at most 3 strips (a strip owns at least one row): 2, and 3 of one row each
    out += [("3x70 in 2", wide3, NODATA, [(0, 1), (1, 3)]), ("3x70 in 3", wide3, NODATA, [(0, 1), (1, 2), (2, 3)])]
    return out


@pytest.mark.parametrize("i", range(8))
def test_strips_equal_the_whole_raster(ctx, restate, base, i):
    label, z, nd, parts = _strip_rasters(base)[i]
    want = restate.run(z, nd)
    assert np.array_equal(_dev(ctx, z, nd), want), label
    ss, w = _in_strips(z, nd, parts)
    assert np.array_equal(ss, want), (label, parts, np.argwhere(ss != want)[:5].tolist())
    assert np.array_equal(w, want.astype(np.float32)), label
    if z.shape[0] > 3:
        assert want.any()


@pytest.mark.parametrize("seed", range(8))
def test_random_cuts_of_a_fractal_with_holes(ctx, oracle, restate, seed):
    rng = np.random.default_rng(900 + seed)
    ny, nx = 200 + int(rng.integers(0, 9)), 300 + int(rng.integers(0, 9))
    z = oracle.synth_dem((ny, nx), 500 + seed)
    for _ in range(10):
        y, x = int(rng.integers(0, ny)), int(rng.integers(0, nx))
        z[max(y - 3, 0):y + 4, max(x - 5, 0):x + 6] = NODATA
    world = int(rng.integers(2, 7))
    cuts = sorted(rng.choice(np.arange(1, ny), world - 1, replace=False).tolist())
    parts = list(zip([0] + cuts, cuts + [ny]))
    want = restate.run(z, NODATA)
    ss, _ = _in_strips(z, NODATA, parts)
    assert np.array_equal(ss, want), (parts, np.argwhere(ss != want)[:5].tolist())
    assert np.array_equal(_dev(ctx, z, NODATA), want)


# ---- the chain: fel -> ss -> ssa -> drop analysis -> threshold, all on the device ----------------------------------------------------------------
def test_chain_to_the_threshold_on_the_device(ctx, oracle, tmp_path):
    """on `plain`.  The DropAnalysis results are held to the restatement of tests/dropan_model.py with the bounds of tests/test_gpu_dropan.py: counts
    exact, each fp64 sum within gamma_n * sum|x| of the correctly rounded sum, the length within gamma relative, the written rows the same."""
    import torch

    g = DM.load_golden("plain")
    par, st = (1.0, 30.0, 10), 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    fel, p, ad8 = dev(g["fel"]), dev(g["p"]), dev(g["ad8"])
    ss, w = ctx.peukerdouglas(fel, float_weights=True)
    assert np.array_equal(ss.cpu().numpy(), M.load_golden("plain")["fel_default"])
    ssa = ctx.aread8(p, weights=w, contcheck=False)
    want_ssa = oracle.aread8(g["p"], -32768, weights=ss.cpu().numpy().astype(np.float32), contcheck=False)
    assert np.array_equal(ssa.cpu().numpy().view(np.uint32), want_ssa.view(np.uint32))
    thresh, n1, n2, sums, length, area, table, opt = ctx.dropanalysis(ad8, p, fel, ssa, (g["cols"], g["rows"]), thresh_min=par[0], thresh_max=par[1], nthresh=par[2],
                                                                      steptype=st, dx=g["dxc"], dy=g["dyc"])
    ref = DM.compile(tmp_path).run(g["ad8"], g["p"], g["fel"], want_ssa, g["cols"], g["rows"], g["dxc"], g["dyc"], par[0], par[1], par[2], st)
    ny = g["p"].shape[0]
    assert np.array_equal(thresh.view(np.uint32), ref["thresh"].view(np.uint32))
    assert np.float32(area) == np.float32(ref["total_area"])
    for th, q in enumerate(ref["per"]):
        assert (int(n1[th]), int(n2[th])) == (q["n1"], q["n2"]), th
        exact, mag = DM.sums_from_drops(q["drops1"], q["drops2"]), DM.abs_sums_from_drops(q["drops1"], q["drops2"])
        for k, nterms in enumerate((q["n1"], q["n1"], q["n2"], q["n2"])):
            assert abs(float(sums[th, k]) - exact[k]) <= DM.gamma(max(nterms, 1)) * mag[k], (th, k, sums[th, k], exact[k])
        want_len, links = DM.exact_length(q["order"], g["p"], g["dxc"], g["dyc"])
        assert abs(float(length[th]) - want_len) <= DM.gamma(links + 3 * ny) * want_len, (th, length[th], want_len)
    got_rows, got_opt = DM.parse_table(table.encode())
    want_rows, want_opt = DM.parse_table(ref["table"])
    assert np.array_equal(got_rows[:, [0, 2, 3]], want_rows[:, [0, 2, 3]]) and len(got_rows) >= 6
    assert opt is not None and np.float32(opt) == ref["optimum"] and got_opt == want_opt and opt > thresh[0]
    src = ctx.threshold(ssa, float(opt)).cpu().numpy()
    want_src = np.where(want_ssa == -1.0, -32768, (want_ssa >= np.float32(opt)).astype(np.int16)).astype(np.int16)
    assert np.array_equal(src, want_src) and (src == 1).any()


# ---- command line -----------------------------------------------------------------------------------------------------------------------------
def _gt(g):
    dx, dy, ny = float(g["dx"]), float(g["dy"]), g["fel"].shape[0]
    return (1000.0, dx, 0.0, 5000.0 + dy * ny, 0.0, -dy)


@pytest.mark.parametrize("gpus", [1, 2])
def test_cli_writes_the_reference_raster(ctx, tmp_path, gpus):
    g = np.load(os.path.join(M.GOLDEN, "case_plain.npz"))
    gold = M.load_golden("plain")
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("fel.tif"), g["fel"], float(T.FEL_NODATA), geotransform=_gt(g))
    r = subprocess.run([os.path.join(BIN, "peukerdouglas"), "--gpus", str(gpus), "-fel", f("fel.tif"), "-ss", f("ss.tif")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PeukerDouglas version" in r.stdout and f"Processors: {gpus}" in r.stdout, r.stdout + r.stderr
    ss, info = T.read_raster(f("ss.tif"), np.int16)
    assert np.array_equal(ss, gold["fel_default"]) and float(info["nodata"]) == -2.0 and M.tiff_sample_type(f("ss.tif")) == (16, 2)
    assert info["geotransform"] == T.raster_info(f("fel.tif"))["geotransform"]
    T.write_raster(f("dem.tif"), g["dem"], float(g["nodata"]), geotransform=_gt(g))
    w = M.PARS[0]
    r = subprocess.run([os.path.join(BIN, "peukerdouglas"), "-par", *[repr(v) for v in w], "-ss", f("ssp.tif"), "--gpus", str(gpus), "-fel", f("dem.tif")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(T.read_raster(f("ssp.tif"), np.int16)[0], gold["dem_par0"])


def test_cli_simple_use_usage_and_errors(ctx, tmp_path):
    g = np.load(os.path.join(M.GOLDEN, "case_plain.npz"))
    gold = M.load_golden("plain")
    f = lambda s: str(tmp_path / s)  # noqa: E731
    exe = os.path.join(BIN, "peukerdouglas")
    T.write_raster(f("basefel.tif"), g["fel"], float(T.FEL_NODATA), geotransform=_gt(g))
    r = subprocess.run([exe, f("base.tif")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(T.read_raster(f("basess.tif"), np.int16)[0], gold["fel_default"])
    # a -par cut short, an unknown flag, no argument: the reference's usage text, exit 0, nothing written
    for args in (["-fel", f("basefel.tif"), "-ss", f("no.tif"), "-par", "0.4", "0.1"], ["-fel", f("basefel.tif"), "-src", f("no.tif")], []):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("Simple Use:") and "Default weights are 0.4 0.1 0.05 if -par is not specified." in r.stdout, args
        assert not os.path.exists(f("no.tif"))
    # an input file that is missing: the ToolRun frame's status for it, from the program and from the Python tool function
    r = subprocess.run([exe, "-fel", f("nope.tif"), "-ss", f("no.tif")], capture_output=True, text=True, timeout=120)
    assert r.returncode == _lib.TDX_ERR_FILE and "Error opening file" in r.stdout and not os.path.exists(f("no.tif"))
    assert tools.peukerdouglas(f("nope.tif"), f("no.tif")) == _lib.TDX_ERR_FILE
    assert tools.peukerdouglas(f("basefel.tif"), f("tool.tif"), M.PARS[1]) == 0
    assert np.array_equal(T.read_raster(f("tool.tif"), np.int16)[0], M.Restatement.run(M.compile(tmp_path), g["fel"], M.FEL_NODATA, M.PARS[1]))
