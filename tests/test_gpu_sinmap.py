"""SinmapSI on the GPU (taudem_amd/csrc/sinmap.hip) against the real tool's rasters (tests/golden/sinmap_*.npz) where there is one, and against the
"double" restatement elsewhere (tests/sinmap_model.py, held to those rasters bit for bit by tests/test_sinmap_restatement.py).

The rule (sinmap_model.check): nodata, not-written and s == 0 cells, the si == 10 cap, sat == 2 and sat == 3 and the NaN pattern are exact; elsewhere sat
is within one float ulp and |si - golden| <= max(one float ulp of the golden, 8 * E_abs), E_abs being what the restatement's variants measured for the case
the cells come from.  Where the same code runs on the same cells - host form against device form, strips against one device, the A/B variants - equality
of bits is required.  Every test prints the largest |si - golden| it measured before it asserts."""
import os
import subprocess

import numpy as np
import pytest

import peuker_model as PM
import sinmap_model as M
import taudem_amd as T
from taudem_amd import _lib, tools

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")
SHAPES = ((1, 1), (1, 7), (5, 3), (33, 67), (96, 127), (96, 128))   # below one lane's four cells, a partial last group, more than one block, a whole number of blocks


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("sinmap"))


@pytest.fixture(scope="module")
def plain():
    """the run every crop is taken from: `plain` (96 x 128) with both roads, and the E_abs of its golden"""
    return dict(M.golden_runs("plain"))["roads"], M.load_golden("plain")[1]["E_abs"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _args(r):
    return (r["regions"], r["rminter"], r["rmaxter"], r["g"], r["rhow"]), {"cal_nodata": r["cal_nodata"], "slp_nodata": float(r["slp_nodata"])}


def _host(ctx, r, **kw):
    a, k = _args(r)
    return ctx.sinmapsi(r["slp"], r["sca"], r["cal"], *a, scamin=r["scamin"], scamax=r["scamax"], **k, **kw)


def _dev(ctx, r, **kw):
    import torch

    d = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    a, k = _args(r)
    si, sat = ctx.sinmapsi(d(r["slp"]), d(r["sca"]), d(r["cal"]), *a, scamin=d(r["scamin"]), scamax=d(r["scamax"]), **k, **kw)
    return si.cpu().numpy(), sat.cpu().numpy()


def _crop(r, ny, nx):
    c = dict(r)
    for k in ("slp", "sca", "cal", "scamin", "scamax"):
        c[k] = None if r[k] is None else np.ascontiguousarray(r[k][:ny, :nx])
    return c


def _expect(restate, r):
    si, sat, code = restate.run("double", r)
    return {"si": si, "sat": sat, "code": code}


# ---- goldens --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES + ("patho",))
def test_every_golden_run_against_the_reference(ctx, case):
    gold, meta = M.load_golden(case)
    worst = 0.0
    for key, r in (M.patho_runs() if case == "patho" else M.golden_runs(case)):
        si, sat = _host(ctx, r)
        dsi, dsat = _dev(ctx, r)
        assert np.array_equal(_bits(si), _bits(dsi)) and np.array_equal(_bits(sat), _bits(dsat)), (case, key, "host form and device form differ")
        codes = gold[key]["code"]
        for k in np.unique(codes[codes >= M.UNSTABLE]).tolist():   # the figure per path, printed before anything is asserted
            m = (codes == k) & np.isfinite(gold[key]["si"]) & np.isfinite(si)
            if m.any():
                print(f"sinmap {case} {key} path {k}: max |si - golden| = {np.abs(si[m].astype(np.float64) - gold[key]['si'][m]).max():.3e} over {int(m.sum())} cells")
        worst = max(worst, M.check(si, sat, gold[key], meta["E_abs"], f"{case} {key}"))
    print(f"sinmap {case}: worst |si - golden| = {worst:.3e}, E_abs = {meta['E_abs']:.3e}, bound 8 * E_abs = {8 * meta['E_abs']:.3e}")


# ---- shapes at the kernel's seams -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_seam_shapes(ctx, restate, plain, shape):
    r, e_abs = _crop(plain[0], *shape), plain[1]
    want = _expect(restate, r)
    si, sat = _dev(ctx, r)
    print(f"sinmap crop {shape}: worst |si - golden| = {M.check(si, sat, want, e_abs, str(shape)):.3e}")
    hsi, hsat = _host(ctx, r)
    assert np.array_equal(_bits(si), _bits(hsi)) and np.array_equal(_bits(sat), _bits(hsat))


@pytest.mark.parametrize("offsets", [(1, 1, 1, 1, 1, 1, 1), (3, 2, 1, 0, 3, 1, 2), (0, 0, 0, 0, 2, 0, 0), (0, 4, 0, 0, 4, 0, 1)])
def test_rasters_at_odd_element_offsets_inside_larger_arrays(ctx, plain, offsets):
    """each raster a contiguous crop that starts `offset` elements into a larger device array: no 16-byte (cal: 8-byte) alignment, each array on its own;
    equal to the aligned call bit for bit, and nothing written outside the crop"""
    import torch

    r = _crop(plain[0], 33, 67)
    n = 33 * 67
    want_si, want_sat = _dev(ctx, r)

    def place(a, off, fill):
        big = torch.full((n + 16,), fill, dtype=torch.from_numpy(a).dtype, device="cuda")
        big[off:off + n] = torch.from_numpy(a.reshape(-1)).cuda()
        return big, big[off:off + n].view(33, 67)

    ins = [place(r[k], off, 7) for k, off in zip(("slp", "sca", "scamin", "scamax", "cal"), offsets)]
    (bsi, vsi), (bsat, vsat) = place(np.zeros((33, 67), np.float32), offsets[5], 777.0), place(np.zeros((33, 67), np.float32), offsets[6], 777.0)
    a, k = _args(r)
    ctx.sinmapsi(ins[0][1], ins[1][1], ins[4][1], *a, scamin=ins[2][1], scamax=ins[3][1], out=(vsi, vsat), **k)
    assert np.array_equal(_bits(vsi.cpu().numpy()), _bits(want_si)) and np.array_equal(_bits(vsat.cpu().numpy()), _bits(want_sat))
    for big, off in ((bsi, offsets[5]), (bsat, offsets[6])):
        rest = torch.cat([big[:off], big[off + n:]]).cpu().numpy()
        assert np.all(rest == 777.0)


def test_each_road_raster_alone(ctx, restate, plain):
    r, e_abs = plain
    for keep in ("scamin", "scamax"):
        one = dict(r)
        one["scamax" if keep == "scamin" else "scamin"] = None
        want = _expect(restate, one)
        si, sat = _dev(ctx, one)
        print(f"sinmap {keep} alone: worst |si - golden| = {M.check(si, sat, want, e_abs, keep):.3e}")
        assert not np.array_equal(_bits(si), _bits(_dev(ctx, r)[0]))


def test_variants_of_the_pass_give_the_same_bits(ctx, plain, monkeypatch):
    for r in (plain[0], _crop(plain[0], 33, 67)):   # many blocks; three blocks and a partial last group of four
        si, sat = _dev(ctx, r)
        _, _, st = ctx.sinmapsi(r["slp"], r["sca"], r["cal"], *_args(r)[0], stats=True)
        assert st["launches_stencil"] == 2
        monkeypatch.setenv("TDX_SINMAP_ONEPASS", "1")
        vsi, vsat = _dev(ctx, r)
        assert np.array_equal(_bits(vsi), _bits(si)) and np.array_equal(_bits(vsat), _bits(sat))
        _, _, st = ctx.sinmapsi(r["slp"], r["sca"], r["cal"], *_args(r)[0], stats=True)
        assert st["launches_stencil"] == 1
        monkeypatch.delenv("TDX_SINMAP_ONEPASS")


def test_out_arguments_regions_forms_and_refusals(ctx, plain, tmp_path):
    r = _crop(plain[0], 20, 30)
    si, sat = np.zeros((20, 30), np.float32), np.zeros((20, 30), np.float32)
    a, k = _args(r)
    got = ctx.sinmapsi(r["slp"], r["sca"], r["cal"], *a, scamin=r["scamin"], scamax=r["scamax"], out=(si, sat), **k)
    assert got[0] is si and got[1] is sat and (si > 0).any()
    path = tmp_path / "calpar.csv"
    path.write_text(r["calpar"])
    rows = [tuple(r["regions"][f][i] for f in M.FIELDS) for i in range(len(r["regions"]["id"]))]
    for regions in (str(path), rows):
        s2, t2 = ctx.sinmapsi(r["slp"], r["sca"], r["cal"], regions, *a[1:], scamin=r["scamin"], scamax=r["scamax"], **k)
        assert np.array_equal(_bits(s2), _bits(si)) and np.array_equal(_bits(t2), _bits(sat))
    s3, t3 = T.sinmapsi(r["slp"], r["sca"], r["cal"], *a, scamin=r["scamin"], scamax=r["scamax"], **k)
    assert np.array_equal(_bits(s3), _bits(si)) and np.array_equal(_bits(t3), _bits(sat))
    for bad in ({"slp": r["slp"].astype(np.float64)}, {"cal": r["cal"].astype(np.int32)}, {"sca": r["sca"][:, ::2]}, {"scamin": r["scamin"][:10]}):
        b = {**r, **bad}
        with pytest.raises(ValueError):
            ctx.sinmapsi(b["slp"], b["sca"], b["cal"], *a, scamin=b["scamin"], scamax=b["scamax"])
    # no region at all: every cell is nodata
    none, _ = ctx.sinmapsi(r["slp"], r["sca"], r["cal"], [], *a[1:])
    assert np.all(none == -1.0)


# ---- strips -----------------------------------------------------------------------------------------------------------------------------------
def _in_strips(r, parts):
    """(si, sat) of run r cut into the row strips `parts` ([(y0, y1)]), each through tdx_sinmapsi_strip on a rank of its own: the owned rows, concatenated.
    The halo rows of the inputs hold junk and those of the outputs a mark that must still be there afterwards."""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline

    nx = r["slp"].shape[1]
    a, k = _args(r)
    with StripGroup(len(parts), nx, [0] * len(parts)) as grp:
        def rank_main(rank, c, comm):
            y0, y1 = parts[rank]
            pipe = StripPipeline(c, comm, nx, y1 - y0)

            def strip(x, dtype, fill):
                if x is None:
                    return None
                t = pipe.empty(dtype)
                t.fill_(fill)
                t[1:y1 - y0 + 1] = torch.from_numpy(np.ascontiguousarray(x[y0:y1])).cuda()
                return t
            si, sat = pipe.empty(torch.float32), pipe.empty(torch.float32)
            si.fill_(777.0)
            sat.fill_(777.0)
            out = pipe.sinmapsi(strip(r["slp"], torch.float32, 0.5), strip(r["sca"], torch.float32, 50.0), strip(r["cal"], torch.int16, 1), *a,
                                scamin=strip(r["scamin"], torch.float32, 0.01), scamax=strip(r["scamax"], torch.float32, 0.02), out=(si, sat), **k)
            assert out[0] is si and out[1] is sat
            halo = torch.cat([si[0], si[-1], sat[0], sat[-1]]).cpu().numpy()
            assert np.all(halo == 777.0), "a halo row of an output was written"
            return si[1:y1 - y0 + 1].cpu().numpy(), sat[1:y1 - y0 + 1].cpu().numpy()
        res = grp.run(rank_main)
    return np.concatenate([x[0] for x in res], axis=0), np.concatenate([x[1] for x in res], axis=0)


def _cuts(ny):
    from taudem_amd.distributed import partition_rows

    rng = np.random.default_rng(31 + ny)
    out = [partition_rows(ny, 2), partition_rows(ny, 3), [(0, 1), (1, ny)], [(0, ny - 1), (ny - 1, ny)], [(0, 40), (40, 41), (41, ny)]]
    for _ in range(3):
        world = int(rng.integers(2, 7))
        cuts = sorted(rng.choice(np.arange(1, ny), world - 1, replace=False).tolist())
        out.append(list(zip([0] + cuts, cuts + [ny])))
    return out


@pytest.mark.parametrize("i", range(8))
def test_strips_equal_the_whole_raster_bit_for_bit(ctx, i):
    """`holes` (120 x 100: rows of 100 cells put every strip but the first at a start that is no multiple of four cells from the array's) with both roads,
    cut into 2 and 3, with one-row strips at the top, the bottom and in the middle, and at random"""
    r = dict(M.golden_runs("holes"))["roads"]
    parts = [tuple(p) for p in _cuts(r["slp"].shape[0])[i]]
    want_si, want_sat = _dev(ctx, r)
    si, sat = _in_strips(r, parts)
    assert np.array_equal(_bits(si), _bits(want_si)) and np.array_equal(_bits(sat), _bits(want_sat)), parts


def test_strips_of_a_raster_with_odd_row_length_and_one_road(ctx, plain):
    r = _crop(plain[0], 33, 67)
    r["scamin"] = None
    want_si, want_sat = _dev(ctx, r)
    for parts in ([(0, 16), (16, 33)], [(0, 1), (1, 2), (2, 33)]):
        si, sat = _in_strips(r, parts)
        assert np.array_equal(_bits(si), _bits(want_si)) and np.array_equal(_bits(sat), _bits(want_sat)), parts


# ---- the chain: fel -> slp, ang -> sca -> si, sat, all on the device ----------------------------------------------------------------------------
def test_chain_from_the_elevations_on_the_device(ctx):
    import torch

    g = np.load(os.path.join(M.GOLDEN, "case_plain.npz"))
    r = dict(M.golden_runs("plain"))["noroads"]
    fel = torch.from_numpy(g["fel"]).cuda()
    ang, slp = ctx.dinfflowdir(fel, dx=g["dxc"], dy=g["dyc"])
    sca = ctx.areadinf(ang, dx=g["dxc"], dy=g["dyc"])
    cal = torch.from_numpy(r["cal"]).cuda()
    a, _ = _args(r)
    si, sat = ctx.sinmapsi(slp, sca, cal, *a)
    assert si.is_cuda and sat.is_cuda and si.dtype == torch.float32
    hsi, hsat = ctx.sinmapsi(slp.cpu().numpy(), sca.cpu().numpy(), r["cal"], *a)
    assert np.array_equal(_bits(si.cpu().numpy()), _bits(hsi)) and np.array_equal(_bits(sat.cpu().numpy()), _bits(hsat))
    live = hsi != -1.0
    assert 0.3 < live.mean() < 1.0 and ((hsi > 0) & (hsi < 1)).any() and (hsat[live] <= 3.0).all()


# ---- command line -----------------------------------------------------------------------------------------------------------------------------
def _write_inputs(d, r):
    f = lambda s: os.path.join(str(d), s)  # noqa: E731
    gt = (1000.0, 30.0, 0.0, 5000.0 + 30.0 * r["slp"].shape[0], 0.0, -30.0)
    T.write_raster(f("slp.tif"), r["slp"], float(r["slp_nodata"]), geotransform=gt)
    T.write_raster(f("sca.tif"), r["sca"], -1.0, geotransform=gt)
    T.write_raster(f("cal.tif"), r["cal"], float(r["cal_nodata"]), geotransform=gt)
    T.write_raster(f("scamin.tif"), r["scamin"], -1.0, geotransform=gt)
    T.write_raster(f("scamax.tif"), r["scamax"], -1.0, geotransform=gt)
    open(f("calpar.csv"), "w").write(r["calpar"])
    return f


PAR = [repr(M.RMINTER), repr(M.RMAXTER), repr(M.G), repr(M.RHOW)]


def _check_files(f, si_name, sat_name, want):
    si, info = T.read_raster(f(si_name), np.float32)
    sat, info2 = T.read_raster(f(sat_name), np.float32)
    assert np.array_equal(_bits(si), _bits(want[0])) and np.array_equal(_bits(sat), _bits(want[1]))
    # what the golden files are: float32 samples, nodata -1, the slope file's georeferencing
    assert float(info["nodata"]) == -1.0 and float(info2["nodata"]) == -1.0
    assert PM.tiff_sample_type(f(si_name)) == (32, 3) and PM.tiff_sample_type(f(sat_name)) == (32, 3)
    assert info["geotransform"] == T.raster_info(f("slp.tif"))["geotransform"]


@pytest.mark.parametrize("gpus", [1, 2])
def test_cli_three_argument_forms(ctx, plain, tmp_path, gpus):
    r = plain[0]
    f = _write_inputs(tmp_path, r)
    exe = os.path.join(BIN, "sinmapsi")
    no_roads = _host(ctx, {**r, "scamin": None, "scamax": None})
    roads = _host(ctx, r)
    run = lambda args: subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)  # noqa: E731
    # 10 positional arguments
    p = run(["--gpus", str(gpus), f("slp.tif"), f("sca.tif"), f("calpar.csv"), f("cal.tif"), f("si10.tif"), f("sat10.tif"), *PAR])
    assert p.returncode == 0 and "SinmapSI version" in p.stdout and "Compute time: " in p.stdout and "File write time: " in p.stdout, p.stdout + p.stderr
    assert "This run may take on the order of 1 minutes to complete." in p.stderr
    _check_files(f, "si10.tif", "sat10.tif", no_roads)
    # 12 positional arguments
    p = run([f("slp.tif"), f("sca.tif"), f("calpar.csv"), f("cal.tif"), f("si12.tif"), f("sat12.tif"), *PAR, f("scamin.tif"), f("scamax.tif"), "--gpus", str(gpus)])
    assert p.returncode == 0, p.stdout + p.stderr
    _check_files(f, "si12.tif", "sat12.tif", roads)
    # flags, in another order
    p = run(["-sat", f("satf.tif"), "-si", f("sif.tif"), "-par", *PAR, "-scamax", f("scamax.tif"), "-cal", f("cal.tif"), "--gpus", str(gpus), "-calpar", f("calpar.csv"),
             "-sca", f("sca.tif"), "-slp", f("slp.tif"), "-scamin", f("scamin.tif")])
    assert p.returncode == 0, p.stdout + p.stderr
    _check_files(f, "sif.tif", "satf.tif", roads)


def test_cli_usage_errors_and_the_tool_function(ctx, plain, tmp_path):
    r = plain[0]
    f = _write_inputs(tmp_path, r)
    exe = os.path.join(BIN, "sinmapsi")
    run = lambda args: subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)  # noqa: E731
    base = ["-slp", f("slp.tif"), "-sca", f("sca.tif"), "-calpar", f("calpar.csv"), "-cal", f("cal.tif"), "-si", f("no.tif"), "-sat", f("nosat.tif")]
    # too few words, 11 arguments, a -par cut short, an unknown flag: the reference's usage text, exit 0, nothing written
    for args in ([], [f("slp.tif")], [f("slp.tif"), f("sca.tif"), f("calpar.csv"), f("cal.tif"), f("no.tif"), f("nosat.tif"), *PAR, f("scamin.tif")],
                 [*base, "-par", "0.0009", "0.00135", "9.81"], [*base, "-par", *PAR, "-road", f("scamin.tif")]):
        p = run(args)
        assert p.returncode == 0 and p.stdout.startswith("Simple Use:") and "<rhow> is the <TODO> constant." in p.stdout, args
        assert not os.path.exists(f("no.tif"))
    # an unreadable -calpar: 15, reported the way the reference's main reports it, exit 0
    p = run([*base[:5], f("nope.csv"), *base[6:], "-par", *PAR])
    assert p.returncode == 0 and "Sinmap Stability Index Error 15" in p.stdout and not os.path.exists(f("no.tif"))
    # a raster of another size: 1, and the sentence naming the two files on stderr
    T.write_raster(f("small.tif"), r["sca"][:10, :10], -1.0, geotransform=(1000.0, 30.0, 0.0, 5300.0, 0.0, -30.0))
    p = run(["-slp", f("slp.tif"), "-sca", f("small.tif"), *base[4:], "-par", *PAR])
    assert p.returncode == 0 and "Sinmap Stability Index Error 1" in p.stdout and not os.path.exists(f("no.tif"))
    assert f"Slope ({f('slp.tif')}) and Contributing area ({f('small.tif')}) files have different dimensions" in p.stderr
    # a missing raster: the frame's status for it
    p = run(["-slp", f("nope.tif"), *base[2:], "-par", *PAR])
    assert p.returncode == _lib.TDX_ERR_FILE and "Error opening file" in p.stdout
    # the Python tool function
    assert tools.sinmapsi(f("slp.tif"), f("sca.tif"), f("cal.tif"), f("calpar.csv"), f("sit.tif"), f("satt.tif"), M.RMINTER, M.RMAXTER, M.G, M.RHOW, f("scamin.tif"),
                          f("scamax.tif")) == 0
    _check_files(f, "sit.tif", "satt.tif", _host(ctx, r))
