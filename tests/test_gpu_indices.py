"""TWI, SlopeArea, SlopeAreaRatio, LengthArea and SetRegion on the GPU (taudem_amd/csrc/indices.hip) against the restatement (tests/indices/indices_restate.c,
compiled on the spot; tests/test_indices_restatement.py holds it to the real tools' rasters): bit for bit, every cell of every tool, on every golden run, every
hand-built raster and at the kernel's seams.  A NaN counts as equal to a NaN at the same place (tests/indices_model.py says why).  Nothing of the reference is
read."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import indices_model as M
import peuker_model as PM
import taudem_amd as T
from taudem_amd import tools

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")
# below one lane's four cells, a partial last group, more than one block, a whole number of blocks; 7, 15 (5 x 3), 2211 and 12192 cells leave the last int16
# group of four (8 bytes) partial, 1 and 12288 do not
SHAPES = ((1, 1), (1, 7), (5, 3), (33, 67), (96, 127), (96, 128))


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("indices"))


@pytest.fixture(scope="module")
def plain():
    return M.case_inputs("plain")


def _gpu(c, tool, r, dev=False):
    """the output of run r through Context c: host arrays, or device tensors"""
    if dev:
        import torch

        r = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v for k, v in r.items()}
    if tool == "twi":
        out = c.twi(r["slp"], r["sca"])
    elif tool == "sar":
        out = c.slopearearatio(r["slp"], r["sca"])
    elif tool == "sa":
        out = c.slopearea(r["slp"], r["sca"], *r["par"])
    elif tool == "la":
        out = c.lengtharea(r["plen"], r["ad8"], *r["par"])
    else:
        out = c.setregion(r["p"], r["gw"], r["id"])
    return out.cpu().numpy() if dev else out


def _crop(r, ny, nx):
    return {k: np.ascontiguousarray(v[:ny, :nx]) if isinstance(v, np.ndarray) else v for k, v in r.items()}


@pytest.mark.parametrize("name", M.FIXTURES)
def test_every_golden_and_hand_built_run_equals_the_restatement(ctx, restate, name):
    runs = M.all_runs(name) + ([M.fractional_run()] if name == "plain" else [])
    for key, tool, r in runs:
        want = restate.run(tool, r)
        got = _gpu(ctx, tool, r)
        assert got.dtype == want.dtype and M.same_bits(got, want), f"{name} {key}: {int(np.sum(got != want))} cells differ from the restatement"
        assert M.same_bits(_gpu(ctx, tool, r, dev=True), got), f"{name} {key}: host form and device form differ"


@pytest.mark.parametrize("shape", SHAPES)
def test_seam_shapes(ctx, restate, plain, shape):
    for key, tool, r in M.crop_runs("plain"):
        r = _crop(r, *shape)
        want = restate.run(tool, r)
        assert M.same_bits(_gpu(ctx, tool, r, dev=True), want), (shape, key)
        assert M.same_bits(_gpu(ctx, tool, r), want), (shape, key, "host form")


def test_every_output_subset_gives_the_bits_of_the_one_output_calls(ctx, plain):
    import torch

    slp, sca = torch.from_numpy(plain["slp"]).cuda(), torch.from_numpy(plain["sca"]).cuda()
    m, n = M.SA_PARS["negexp"]
    one = {"twi": ctx.twi(slp, sca), "sa": ctx.slopearea(slp, sca, m, n), "sar": ctx.slopearearatio(slp, sca)}
    names = ("twi", "sa", "sar")
    for k in (1, 2, 3):
        for want in itertools.permutations(names, k):
            res = ctx.terrain_indices(slp, sca, m, n, want=want)
            res = (res,) if k == 1 else res
            assert len(res) == k
            for w, a in zip(want, res):
                assert torch.equal(a.view(torch.int32), one[w].view(torch.int32)), (want, w)
    *_, st = ctx.terrain_indices(slp, sca, m, n, stats=True)
    assert st["launches_stencil"] == 1   # three outputs, one pass


def test_out_arguments_and_refusals(ctx, plain):
    r = _crop(plain, 20, 30)
    twi, sar = np.zeros((20, 30), np.float32), np.zeros((20, 30), np.float32)
    got = ctx.terrain_indices(r["slp"], r["sca"], want=("sar", "twi"), out=(sar, twi))
    assert got[0] is sar and got[1] is twi and M.same_bits(twi, ctx.twi(r["slp"], r["sca"])) and M.same_bits(sar, ctx.slopearearatio(r["slp"], r["sca"]))
    ss = np.zeros((20, 30), np.int16)
    assert ctx.lengtharea(r["plen"], r["ad8"], out=ss) is ss and (ss == 1).any()
    reg = np.zeros((20, 30), np.int32)
    assert ctx.setregion(r["p"], r["gw"], 9, out=reg) is reg and (reg == 9).any()
    assert M.same_bits(T.terrain_indices(r["slp"], r["sca"], want=("twi",)), twi) and M.same_bits(T.lengtharea(r["plen"], r["ad8"]), ss)
    assert M.same_bits(T.setregion(r["p"], r["gw"], 9), reg)
    for want in ((), ("twi", "twi"), ("tw",)):
        with pytest.raises(ValueError):
            ctx.terrain_indices(r["slp"], r["sca"], want=want)
    with pytest.raises(ValueError):
        ctx.terrain_indices(r["slp"], r["sca"], want=("twi",), out=(twi, sar))
    for call in (lambda: ctx.twi(r["slp"].astype(np.float64), r["sca"]), lambda: ctx.lengtharea(r["plen"], r["ad8"].astype(np.int32)),
                 lambda: ctx.setregion(r["p"].astype(np.int32), r["gw"]), lambda: ctx.slopearea(r["slp"], r["sca"][:10])):
        with pytest.raises(ValueError):
            call()


def test_rasters_at_odd_element_offsets_inside_larger_arrays(ctx, plain):
    """each raster a contiguous crop that starts an odd number of elements into a larger device array: no 16-byte (int16: 8-byte) alignment; equal to the
    aligned call bit for bit, and nothing written outside the crop"""
    import torch

    r = _crop(plain, 33, 67)
    n = 33 * 67

    def place(a, off, fill):
        big = torch.full((n + 16,), fill, dtype=torch.from_numpy(a).dtype, device="cuda")
        big[off:off + n] = torch.from_numpy(a.reshape(-1)).cuda()
        return big, big[off:off + n].view(33, 67)

    for offs in ((1, 3, 1, 2, 3), (0, 0, 2, 0, 1), (3, 1, 0, 0, 0)):
        slp, sca = place(r["slp"], offs[0], 7)[1], place(r["sca"], offs[1], 7)[1]
        outs = [place(np.zeros((33, 67), np.float32), o, 777.0) for o in offs[2:]]
        ctx.terrain_indices(slp, sca, 1.5, -0.75, out=tuple(v for _, v in outs))
        want = ctx.terrain_indices(r["slp"], r["sca"], 1.5, -0.75)
        for (big, v), w, o in zip(outs, want, offs[2:]):
            assert M.same_bits(v.cpu().numpy(), w)
            assert np.all(torch.cat([big[:o], big[o + n:]]).cpu().numpy() == 777.0)
        plen, ad8 = place(r["plen"], offs[0], 7)[1], place(r["ad8"], offs[1], 7)[1]
        big, ss = place(np.zeros((33, 67), np.int16), offs[2], 777)
        ctx.lengtharea(plen, ad8, out=ss)
        assert M.same_bits(ss.cpu().numpy(), ctx.lengtharea(r["plen"], r["ad8"])) and np.all(torch.cat([big[:offs[2]], big[offs[2] + n:]]).cpu().numpy() == 777)
        p, gw = place(r["p"], offs[0], 1)[1], place(r["gw"], offs[1], 1)[1]
        big, reg = place(np.zeros((33, 67), np.int32), offs[2], 777)
        ctx.setregion(p, gw, 4, out=reg)
        assert M.same_bits(reg.cpu().numpy(), ctx.setregion(r["p"], r["gw"], 4)) and np.all(torch.cat([big[:offs[2]], big[offs[2] + n:]]).cpu().numpy() == 777)


def test_chain_on_the_device(ctx):
    """dinfflowdir -> areadinf -> terrain_indices and d8flowdir -> aread8 / gridnet -> lengtharea without a raster leaving the device"""
    import torch

    g = np.load(os.path.join(M.GOLDEN, "case_plain.npz"))
    fel = torch.from_numpy(g["fel"]).cuda()
    ang, slp = ctx.dinfflowdir(fel, dx=g["dxc"], dy=g["dyc"])
    sca = ctx.areadinf(ang, dx=g["dxc"], dy=g["dyc"])
    twi, sa, sar = ctx.terrain_indices(slp, sca)
    assert twi.is_cuda and sa.is_cuda and sar.is_cuda and (twi.cpu().numpy() != -1).mean() > 0.5
    p, _ = ctx.d8flowdir(fel, dx=g["dxc"], dy=g["dyc"])
    ad8 = ctx.aread8(p)
    plen = ctx.gridnet(p, dx=g["dxc"], dy=g["dyc"])[0]
    ss = ctx.lengtharea(plen, ad8).cpu().numpy()
    assert set(np.unique(ss).tolist()) == {-32768, 0, 1}


# ---- command line -----------------------------------------------------------------------------------------------------------------------------
GT = lambda ny: (1000.0, 30.0, 0.0, 5000.0 + 30.0 * ny, 0.0, -30.0)  # noqa: E731
GT2 = lambda ny: (2000.0, 30.0, 0.0, 5000.0 + 30.0 * ny, 0.0, -30.0)  # noqa: E731  (the second input's: whose georeferencing the output takes shows)


def _write(d, i):
    f = lambda s: os.path.join(str(d), s)  # noqa: E731
    ny = i["slp"].shape[0]
    T.write_raster(f("slp.tif"), i["slp"], -1.0, geotransform=GT(ny))
    T.write_raster(f("sca.tif"), i["sca"], -1.0, geotransform=GT2(ny))
    T.write_raster(f("plen.tif"), i["plen"], -1.0, geotransform=GT(ny))
    T.write_raster(f("ad8.tif"), i["ad8"].astype(np.int32), -1, geotransform=GT2(ny))
    T.write_raster(f("p.tif"), i["p"], -32768, geotransform=GT(ny))
    T.write_raster(f("gw.tif"), i["gw"], -2147483647, geotransform=GT2(ny))
    return f


def _cli_runs(f, suffix):
    """tool -> (arguments, output file, banner)"""
    o = lambda t: f(f"{t}{suffix}.tif")  # noqa: E731
    return {"twi": (["-slp", f("slp.tif"), "-sca", f("sca.tif"), "-twi", o("twi")], o("twi"), "Topographic Wetness Index version"),
            "slopearea": (["-sa", o("slopearea"), "-par", "1.5", "-0.75", "-sca", f("sca.tif"), "-slp", f("slp.tif")], o("slopearea"), "SlopeArea version"),
            "slopearearatio": (["-sca", f("sca.tif"), "-slp", f("slp.tif"), "-sar", o("slopearearatio")], o("slopearearatio"), "SlopeAreaRatio version"),
            "lengtharea": (["-plen", f("plen.tif"), "-ad8", f("ad8.tif"), "-ss", o("lengtharea")], o("lengtharea"), "LengthArea version"),
            "setregion": (["-p", f("p.tif"), "-gw", f("gw.tif"), "-out", o("setregion"), "-id", "7"], o("setregion"), "SetRegion version")}


def _expected(ctx, i):
    """tool -> (array, numpy dtype, nodata, (bits, sample format) of the file, the input whose georeferencing the output takes)"""
    return {"twi": (ctx.twi(i["slp"], i["sca"]), np.float32, -1.0, (32, 3), "slp.tif"),
            "slopearea": (ctx.slopearea(i["slp"], i["sca"], 1.5, -0.75), np.float32, -1.0, (32, 3), "slp.tif"),
            "slopearearatio": (ctx.slopearearatio(i["slp"], i["sca"]), np.float32, -1.0, (32, 3), "slp.tif"),
            "lengtharea": (ctx.lengtharea(i["plen"], i["ad8"]), np.int16, -32768.0, (16, 2), "ad8.tif"),
            "setregion": (ctx.setregion(i["p"], i["gw"], 7), np.int32, -2147483647.0, (32, 2), "gw.tif")}


def _check_file(f, path, want):
    arr, dtype, nodata, sample, like = want
    got, info = T.read_raster(path, dtype)
    assert M.same_bits(got, arr), path
    assert float(info["nodata"]) == nodata and PM.tiff_sample_type(path) == sample
    assert info["geotransform"] == T.raster_info(f(like))["geotransform"]


def test_cli_files_equal_the_context_arrays(ctx, plain, tmp_path):
    f = _write(tmp_path, plain)
    want = _expected(ctx, plain)
    for tool, (args, out, banner) in _cli_runs(f, "").items():
        p = subprocess.run([os.path.join(BIN, tool), *args], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and banner in p.stdout and "Compute time: " in p.stdout, tool + p.stdout + p.stderr
        assert ("Time estimate not available." if tool == "setregion" else "This run may take on the order of 1 minutes to complete.") in p.stderr
        _check_file(f, out, want[tool])


def test_cli_simple_use_defaults_and_refusals(ctx, plain, tmp_path):
    f = _write(tmp_path, plain)
    # simple use: base name + the reference's suffixes; -par defaults 2 1 and 0.03 1.3, -id default 1
    for name in ("slp", "sca", "plen", "ad8"):
        os.rename(f(name + ".tif"), f("base" + name + ".tif"))
    for tool, suffix, want in (("twi", "twi", ctx.twi(plain["slp"], plain["sca"])), ("slopearea", "sa", ctx.slopearea(plain["slp"], plain["sca"])),
                               ("slopearearatio", "sar", ctx.slopearearatio(plain["slp"], plain["sca"])), ("lengtharea", "ss", ctx.lengtharea(plain["plen"], plain["ad8"]))):
        p = subprocess.run([os.path.join(BIN, tool), f("base.tif")], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, tool + p.stdout + p.stderr
        assert M.same_bits(T.read_raster(f("base" + suffix + ".tif"), want.dtype)[0], want), tool
    p = subprocess.run([os.path.join(BIN, "setregion"), "-out", f("reg.tif"), "-gw", f("gw.tif"), "-p", f("p.tif")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and M.same_bits(T.read_raster(f("reg.tif"), np.int32)[0], ctx.setregion(plain["p"], plain["gw"]))
    # a second raster of another size: the four index tools return 1 without a word, SetRegion says so and ends with 5
    T.write_raster(f("small.tif"), plain["sca"][:10, :10], -1.0, geotransform=GT(10))
    T.write_raster(f("smallgw.tif"), plain["gw"][:10, :10], -2147483647, geotransform=GT(10))
    p = subprocess.run([os.path.join(BIN, "twi"), "-slp", f("baseslp.tif"), "-sca", f("small.tif"), "-twi", f("no.tif")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "TWI error 1" in p.stdout and not os.path.exists(f("no.tif"))
    p = subprocess.run([os.path.join(BIN, "lengtharea"), "-plen", f("baseplen.tif"), "-ad8", f("smallgw.tif"), "-ss", f("no.tif")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Length Area Error 1" in p.stdout and not os.path.exists(f("no.tif"))
    p = subprocess.run([os.path.join(BIN, "setregion"), "-p", f("p.tif"), "-gw", f("smallgw.tif"), "-out", f("no.tif")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 5 and "File sizes do not match" in p.stdout and not os.path.exists(f("no.tif"))
    # the Python tool functions
    assert tools.twigrid(f("baseslp.tif"), f("basesca.tif"), f("t.tif")) == 0 and tools.atanbgrid(f("baseslp.tif"), f("basesca.tif"), f("r.tif")) == 0
    assert tools.slopearea(f("baseslp.tif"), f("basesca.tif"), f("a.tif"), (1.5, -0.75)) == 0 and tools.lengtharea(f("baseplen.tif"), f("basead8.tif"), f("l.tif")) == 0
    assert tools.setregion(f("p.tif"), f("gw.tif"), f("s.tif"), 7) == 0
    want = _expected(ctx, plain)
    for name, tool in (("t.tif", "twi"), ("r.tif", "slopearearatio"), ("a.tif", "slopearea"), ("l.tif", "lengtharea"), ("s.tif", "setregion")):
        assert M.same_bits(T.read_raster(f(name), want[tool][1])[0], want[tool][0]), name
