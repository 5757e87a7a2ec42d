"""StreamNet on the GPU (taudem_amd/csrc/streamnet.hip + streamnet_links.cpp): Context.streamnet and the command-line tool against the reference's
one-rank outputs (tests/golden/streamnet_*.npz: the five cases and the hand-built rasters, each without outlets, with outlets and with -sw) - the
-ord and -w rasters exactly, the -tree and -coord files byte for byte - and against the C++ restatement of tests/streamnet_model.py (held to those
goldens by tests/test_streamnet_restatement.py) on generated rasters that no golden covers.  The cases are 100 x 120 and the like (columns x rows): more than one
64 x 64 tile each way, with tile edges that cross streams."""
import os
import subprocess

import numpy as np
import pytest

import streamnet_model as M
import taudem_amd as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("streamnet"))


def case_inputs(name):
    g = M.load_golden(name)
    c = M.case_fields(name)
    return g, dict(p=g["p"], src=g["src"].astype(np.int32), fel=c["fel"], ad8=c["ad8"], dx=c["dxc"], dy=c["dyc"], gt=tuple(g["gt"]), geographic=bool(c["geographic"]),
                   outlets=(g["cols"], g["rows"], g["ids"]))


def small_inputs(name):
    p, src = M.small_rasters()[name]
    fel, ad8 = M.small_fields(p)
    return dict(p=p, src=src.astype(np.int32), fel=fel, ad8=ad8, dx=M.SMALL_DX, dy=M.SMALL_DY, gt=M.SMALL_GT, geographic=False, outlets=M.SMALL_OUTLETS)


def run_context(ctx, i, variant):
    return ctx.streamnet(i["p"], i["src"], i["fel"], i["ad8"], i["outlets"] if variant == "outlets" else None, variant == "sw", dx=i["dx"], dy=i["dy"],
                         geotransform=i["gt"])


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", M.CASES)
def test_context_matches_reference_cases(ctx, name, variant):
    g, i = case_inputs(name)
    M.assert_equals_golden(f"{name}/{variant}", run_context(ctx, i, variant), g, variant)


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", sorted(M.small_rasters()))
def test_context_matches_reference_hand_built(ctx, name, variant):
    g = M.load_golden("small")
    assert name in set(g["names"].tolist()), f"the reference did not finish on {name}"
    M.assert_equals_golden(f"{name}/{variant}", run_context(ctx, small_inputs(name), variant), g, variant, name + "_")


def run_cli(tmp_path, i, variant, gpus=None):
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("p.tif"), i["p"], M.P_NODATA, geotransform=i["gt"], geographic=i["geographic"])
    T.write_raster(f("src.tif"), i["src"].astype(np.int16), M.SRC_NODATA, geotransform=i["gt"], geographic=i["geographic"])
    T.write_raster(f("fel.tif"), i["fel"], -3.0e38, geotransform=i["gt"], geographic=i["geographic"])
    T.write_raster(f("ad8.tif"), i["ad8"], -1.0, geotransform=i["gt"], geographic=i["geographic"])
    gt = i["gt"]
    with open(f("outlets.txt"), "w") as fo:
        for c, r, k in zip(*i["outlets"]):
            fo.write(f"{float(gt[0] + (c + 0.5) * abs(gt[1]))!r} {float(gt[3] - (r + 0.5) * abs(gt[5]))!r} {k}\n")
    args = [os.path.join(BIN, "streamnet")] + (["--gpus", str(gpus)] if gpus else []) + ["-p", f("p.tif"), "-src", f("src.tif"), "-fel", f("fel.tif"), "-ad8", f("ad8.tif"), "-ord", f("ord.tif"), "-w", f("w.tif"),
            "-tree", f("tree.txt"), "-coord", f("coord.txt")] + {"plain": [], "outlets": ["-o", f("outlets.txt")], "sw": ["-sw"]}[variant]
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ordg, _ = T.read_raster(f("ord.tif"), np.int16)
    w, _ = T.read_raster(f("w.tif"), np.int32)
    return ordg, w, open(f("tree.txt"), "rb").read(), open(f("coord.txt"), "rb").read(), r


def assert_files_equal_golden(tag, got, g, variant, prefix=""):
    ordg, w, tree, coord, _ = got
    k = lambda s: f"{prefix}{s}_{variant}"  # noqa: E731
    assert np.array_equal(ordg, g[k("ord")]) and np.array_equal(w, g[k("w")]), tag
    assert tree == bytes(g[k("tree")]), f"{tag}: -tree differs"
    assert coord == bytes(g[k("coord")]), f"{tag}: -coord differs"


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", M.CASES)
def test_cli_matches_reference_cases(tmp_path, name, variant):
    g, i = case_inputs(name)
    got = run_cli(tmp_path, i, variant)
    assert_files_equal_golden(f"{name}/{variant}", got, g, variant)
    assert got[4].stdout.startswith("StreamNet version ") and "Processors: 1\nRead time: " in got[4].stdout


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", sorted(M.small_rasters()))
def test_cli_matches_reference_hand_built(tmp_path, name, variant):
    g = M.load_golden("small")
    assert_files_equal_golden(f"{name}/{variant}", run_cli(tmp_path, small_inputs(name), variant), g, variant, name + "_")


def test_cli_refuses_the_network_layer(tmp_path):
    r = subprocess.run([os.path.join(BIN, "streamnet"), "-p", "p.tif", "-src", "src.tif", "-fel", "fel.tif", "-ad8", "ad8.tif", "-ord", "ord.tif", "-w", "w.tif", "-tree",
                        "tree.txt", "-coord", "coord.txt", "-net", str(tmp_path / "net.shp")], capture_output=True, text=True)
    assert r.returncode != 0 and "-net" in r.stderr and not os.listdir(tmp_path)


def generated(ctx, oracle, shape, seed):
    """p, src, fel, ad8 of a pit-filled synthetic DEM: src = 1 on the top 4 % of AreaD8, a few 2s and nodata holes, a p == 0 stream cell, a 2-cell cycle on the
    stream, outlets."""
    rng = np.random.default_rng(seed)
    ny, nx = shape
    fel = ctx.pitremove(oracle.synth_dem(shape, seed), -9999.0)
    p, _ = ctx.d8flowdir(fel, -3.0e38, 10.0, 12.5)
    p = p.copy()
    ad8 = ctx.aread8(p, contcheck=False)
    src = np.where((ad8 >= np.quantile(ad8, 0.96)) & (p != M.P_NODATA), 1, 0).astype(np.int32)
    on = np.flatnonzero(src == 1)
    src.flat[rng.choice(on, 4, replace=False)] = 2
    src.flat[rng.choice(on, 3, replace=False)] = M.SRC_NODATA
    src[rng.random(shape) < 0.002] = M.SRC_NODATA
    p.flat[rng.choice(np.flatnonzero(src == 1), 1)] = 0
    pairs = np.argwhere((src[:, :-1] == 1) & (src[:, 1:] == 1) & (p[:, :-1] > 0) & (p[:, 1:] > 0))
    y, x = pairs[len(pairs) // 2]
    p[y, x], p[y, x + 1] = 1, 5                                          # a 2-cell cycle on the stream: no length, no link, nothing labelled through it
    picks = rng.choice(np.flatnonzero(src == 1), 6, replace=False)
    outlets = (np.append(picks % nx, [nx + 2, picks[0] % nx]).astype(np.int32), np.append(picks // nx, [3, picks[0] // nx]).astype(np.int32),
               np.array([31, 7, 1002, 5, 77, 12, 9, 400], np.int32))
    return dict(p=p, src=src, fel=fel, ad8=ad8, dx=10.0, dy=12.5, gt=(500.0, 10.0, 0.0, 8000.0, 0.0, -12.5), geographic=False, outlets=outlets)


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("shape", [(65, 129), (130, 150)])
def test_generated_rasters_match_restatement(ctx, oracle, restate, monkeypatch, shape, variant):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    i = generated(ctx, oracle, shape, 11 + shape[0])
    o = i["outlets"] if variant == "outlets" else ((), (), ())
    ref = restate.run(i["p"], i["src"], i["fel"], i["ad8"], i["dx"], i["dy"], M.gt4(i["gt"]), *o, sw=variant == "sw")
    ordg, w, tree, coord = run_context(ctx, i, variant)
    assert len(ref[2]) >= 10, "the generated raster has too few links to say anything"
    assert np.array_equal(ordg, ref[0]) and np.array_equal(w, ref[1]), f"{int(np.sum(ordg != ref[0]))} order cells, {int(np.sum(w != ref[1]))} labels differ"
    assert np.array_equal(tree, ref[2]) and M.coord_text(coord) == M.coord_text(ref[3])


def test_device_tensors_and_phases(ctx):
    import torch

    g, i = case_inputs("holes")
    dev = f"cuda:{ctx.device}"
    t = {k: torch.from_numpy(np.ascontiguousarray(i[k])).to(dev) for k in ("p", "src", "fel", "ad8")}
    ordg, w, tree, coord, ms = ctx.streamnet(t["p"], t["src"], t["fel"], t["ad8"], i["outlets"], dx=i["dx"], dy=i["dy"], geotransform=i["gt"], phases=True)
    assert ordg.is_cuda and w.is_cuda
    M.assert_equals_golden("device tensors", (ordg.cpu().numpy(), w.cpu().numpy(), tree, coord), g, "outlets")
    assert T.streamnet_text(tree, coord) == (bytes(g["tree_outlets"]), bytes(g["coord_outlets"]))
    assert set(ms) == {"setup", "length", "compact", "links", "scatter", "label", "total"} and ms["total"] > 0
