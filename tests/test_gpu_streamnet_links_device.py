"""StreamNet with the links built on the device (taudem_amd/csrc/streamnet_links_device.hip; Context.streamnet(..., links="device"), bin/streamnet -links
device): the reference's one-rank outputs byte for byte on every golden, the host builder's outputs in the same process on the generated and the
pathological rasters, and the serial restatement (tests/streamnet_model.py) on shapes chosen to break the device builder - a serpentine chain that needs
more than eleven jump rounds and crosses every wave and block boundary of the compact arrays, a comb whose link tree is as deep as its stem is long,
junctions of three and four streams with tied orders, a link that ends above a src == 2 cell while the stream goes on, outlets on every kind of cell, a
cycle, no stream cell, nothing but stream cells.  The definition itself is held without a GPU by tests/test_streamnet_links_device_model.py."""
import os
import subprocess

import numpy as np
import pytest

import pathological as PG
import streamnet_model as M
import taudem_amd as T
from test_gpu_streamnet import BIN, assert_files_equal_golden, case_inputs, generated, small_inputs
from test_gpu_streamnet_pathological import patho_case

pytestmark = pytest.mark.gpu
E, N, W, S, SW, SE = 1, 3, 5, 7, 6, 8   # D8 codes
GT = (300.0, 10.0, 0.0, 7000.0, 0.0, -12.5)


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("streamnet_links_device"))


def run_device(ctx, i, variant, links="device", **kw):
    return ctx.streamnet(i["p"], i["src"], i["fel"], i["ad8"], i["outlets"] if variant == "outlets" else None, variant == "sw", dx=i["dx"], dy=i["dy"],
                         geotransform=i["gt"], links=links, **kw)


def assert_same(tag, got, ref):
    assert np.array_equal(got[0], ref[0]), f"{tag}: {int(np.sum(got[0] != ref[0]))} order cells differ"
    assert np.array_equal(got[1], ref[1]), f"{tag}: {int(np.sum(got[1] != ref[1]))} labels differ"
    assert got[2].shape == ref[2].shape and np.array_equal(got[2], ref[2]), f"{tag}: tree rows differ"
    assert got[3].shape == ref[3].shape and np.array_equal(got[3].view(np.uint64), ref[3].view(np.uint64)), f"{tag}: coord rows differ"


# ---- goldens ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", M.CASES)
def test_context_matches_reference_cases(ctx, name, variant):
    g, i = case_inputs(name)
    M.assert_equals_golden(f"{name}/{variant}", run_device(ctx, i, variant), g, variant)


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", sorted(M.small_rasters()))
def test_context_matches_reference_hand_built(ctx, name, variant):
    g = M.load_golden("small")
    M.assert_equals_golden(f"{name}/{variant}", run_device(ctx, small_inputs(name), variant), g, variant, name + "_")


def run_cli(tmp_path, i, variant, links, gpus=None):
    f = lambda s: str(tmp_path / s)  # noqa: E731
    T.write_raster(f("p.tif"), i["p"], M.P_NODATA, geotransform=i["gt"], geographic=i["geographic"])
    T.write_raster(f("src.tif"), i["src"].astype(np.int16), M.SRC_NODATA, geotransform=i["gt"], geographic=i["geographic"])
    T.write_raster(f("fel.tif"), i["fel"], -3.0e38, geotransform=i["gt"], geographic=i["geographic"])
    T.write_raster(f("ad8.tif"), i["ad8"], -1.0, geotransform=i["gt"], geographic=i["geographic"])
    gt = i["gt"]
    with open(f("outlets.txt"), "w") as fo:
        for c, r, k in zip(*i["outlets"]):
            fo.write(f"{float(gt[0] + (c + 0.5) * abs(gt[1]))!r} {float(gt[3] - (r + 0.5) * abs(gt[5]))!r} {k}\n")
    args = ([os.path.join(BIN, "streamnet")] + (["--gpus", str(gpus)] if gpus else []) + ["-links", links, "-p", f("p.tif"), "-src", f("src.tif"), "-fel", f("fel.tif"),
            "-ad8", f("ad8.tif"), "-ord", f("out_ord.tif"), "-w", f("out_w.tif"), "-tree", f("out_tree.txt"), "-coord", f("out_coord.txt")]
            + {"plain": [], "outlets": ["-o", f("outlets.txt")], "sw": ["-sw"]}[variant])
    r = subprocess.run(args, capture_output=True, text=True)
    if r.returncode != 0:
        return r
    ordg, _ = T.read_raster(f("out_ord.tif"), np.int16)
    w, _ = T.read_raster(f("out_w.tif"), np.int32)
    return ordg, w, open(f("out_tree.txt"), "rb").read(), open(f("out_coord.txt"), "rb").read(), r


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", M.CASES)
def test_cli_matches_reference_cases(tmp_path, name, variant):
    g, i = case_inputs(name)
    got = run_cli(tmp_path, i, variant, "device")
    assert isinstance(got, tuple), got.stdout + got.stderr
    assert_files_equal_golden(f"{name}/{variant}", got, g, variant)


@pytest.mark.parametrize("name", sorted(M.small_rasters()))
def test_cli_matches_reference_hand_built(tmp_path, name):
    g = M.load_golden("small")
    for variant in M.VARIANTS:
        d = tmp_path / variant
        d.mkdir()
        got = run_cli(d, small_inputs(name), variant, "device")
        assert isinstance(got, tuple), got.stdout + got.stderr
        assert_files_equal_golden(f"{name}/{variant}", got, g, variant, name + "_")


# ---- against the host builder ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 129), (130, 150)])
def test_generated_rasters_equal_the_host_builder(ctx, oracle, shape):
    i = generated(ctx, oracle, shape, 11 + shape[0])
    for variant in M.VARIANTS:
        host = run_device(ctx, i, variant, links="host")
        assert len(host[2]) >= 10, "the generated raster has too few links to say anything"
        assert_same(f"{shape}/{variant}", run_device(ctx, i, variant), host)


@pytest.mark.parametrize("name", sorted(PG.CASES))
def test_pathological_rasters_equal_the_host_builder(ctx, oracle, name):
    c = patho_case(oracle, name)
    i = dict(c, dx=30.0, dy=30.0, gt=(100.0, 30.0, 0.0, 9000.0, 0.0, -30.0))
    for variant in M.VARIANTS:
        assert_same(f"{name}/{variant}", run_device(ctx, i, variant), run_device(ctx, i, variant, links="host"))


# ---- shapes chosen to break the device builder -----------------------------------------------------------------------------------------------------
def fields(p, src, outlets=((), (), ())):
    ny, nx = p.shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    fel = (500.0 - 0.75 * yy + 0.125 * np.abs(xx - nx // 3)).astype(np.float32)
    ad8 = (1.0 + (yy * nx + xx) % 977).astype(np.float32)
    o = tuple(np.asarray(a, np.int32) for a in outlets)
    return dict(p=p.astype(np.int16), src=src.astype(np.int32), fel=fel, ad8=ad8, dx=10.0, dy=12.5, gt=GT, geographic=False, outlets=o)


def blank(ny, nx):
    return np.full((ny, nx), S, np.int16), np.zeros((ny, nx), np.int32)


def serpentine(n=64):
    p, src = blank(n, n)
    src[:] = 1
    p[0::2, :] = E
    p[1::2, :] = W
    p[0::2, n - 1] = S
    p[1::2, 0] = S
    p[n - 1, 0 if n % 2 == 0 else n - 1] = W if n % 2 == 0 else E   # the last cell leaves the raster
    return fields(p, src, ([n // 2, 0, n - 1], [n // 2, 0, n - 1], [5, 6, 7]))


def comb(stem=200, seed=5):
    rng = np.random.default_rng(seed)
    p, src = blank(13, stem + 1)
    y = 6
    p[y, :stem] = E
    src[y, :stem] = 1
    for x in range(stem):
        n = int(rng.integers(1, 6))
        src[y - n:y, x] = 1                                  # from the north, flowing south
        if rng.random() < 0.3:                               # now and then one from the south as well: a junction of three, tied orders
            m = int(rng.integers(1, 6))
            src[y + 1:y + 1 + m, x] = 1
            p[y + 1:y + 1 + m, x] = N
    xs = rng.choice(stem, 4, replace=False)
    return fields(p, src, (xs, [y] * 4, [11, 12, 13, 14]))


def junctions():
    """Three junction cells on row 6: inflow orders (1, 1, 1), (1, 2, 2) and (2, 1, 1, 2) in slot order (east, north-east, north, west)."""
    p, src = blank(14, 40)

    def arm(y, x, dy, dx, code, second):
        for k in range(1, 5):
            p[y + k * dy, x + k * dx], src[y + k * dy, x + k * dx] = code, 1
        if second:                                            # a one-cell tributary three cells up the arm: order 2 from there on
            ty, tx, tcode = {E: (y + 1, x - 3, N), W: (y + 1, x + 3, N), S: (y - 3, x + 1, W)}[code]
            p[ty, tx], src[ty, tx] = tcode, 1

    for x, arms in ((7, ((W, 1), (S, 1), (E, 1))), (20, ((W, 1), (S, 2), (E, 2))), (33, ((W, 2), (SW, 1), (S, 1), (E, 2)))):
        src[6:12, x] = 1                                      # the junction and the stream below it, flowing south off the stream
        for code, order in arms:
            dy, dx = {E: (0, -1), W: (0, 1), S: (-1, 0), SW: (-1, 1)}[code]   # where the arm lies, seen from the junction
            arm(6, x, dy, dx, code, order == 2)
    # outlets: on a source, mid-link, on a junction, on a terminal cell, two on one cell, one off the stream
    cols, rows, ids = [3, 5, 7, 7, 20, 20, 0], [6, 6, 6, 11, 9, 9, 0], [31, 32, 33, 34, 35, 36, 37]
    return fields(p, src, (cols, rows, ids))


def src_two_in_mid_stream():
    p, src = blank(40, 9)
    src[2:38, 4] = 1
    src[20, 4] = 2                                            # the cell above it is terminal, the stream goes on
    src[10:20, 2] = 1
    p[19, 2] = E
    p[19, 3], src[19, 3] = E, 1                               # a tributary that joins right at the terminal cell
    return fields(p, src, ([4, 4], [19, 30], [8, 9]))


def cycle():
    p, src = blank(12, 12)
    p[5, 5], p[5, 6] = E, W                                   # two stream cells pointing at each other
    src[5, 5] = src[5, 6] = 1
    src[1:5, 5] = 1                                           # a tributary into them
    src[6:11, 6] = 1                                          # and a stream below them, which starts on its own
    p[5, 8], p[5, 9], src[5, 8], src[5, 9] = E, W, 1, 1       # a cycle of cells with one inflow each and nothing else
    return fields(p, src, ([5, 6], [5, 8], [3, 4]))


def all_stream(n=40):
    p, src = blank(n, n)
    src[:] = 1
    p[:, :n // 2] = SE
    p[:, n // 2:] = SW
    p[n - 1, :] = E
    return fields(p, src, ([n // 2, 3], [n // 2, n - 1], [1, 2]))


def no_stream():
    p, src = blank(33, 70)
    return fields(p, src, ([3], [3], [1]))


SHAPES = {"serpentine": serpentine, "comb": comb, "junctions": junctions, "src_two_in_mid_stream": src_two_in_mid_stream, "cycle": cycle, "all_stream": all_stream,
          "no_stream": no_stream}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_match_the_restatement(ctx, restate, name):
    i = SHAPES[name]()
    for variant in ("plain", "outlets"):
        o = i["outlets"] if variant == "outlets" else ((), (), ())
        ref = restate.run(i["p"], i["src"], i["fel"], i["ad8"], i["dx"], i["dy"], M.gt4(i["gt"]), *o)
        assert_same(f"{name}/{variant}", run_device(ctx, i, variant), ref)
    if name == "junctions":
        orders = {x: sorted(int(ref[0][y, xx]) for y, xx in cells) for x, cells in
                  ((7, ((6, 6), (5, 7), (6, 8))), (20, ((6, 19), (5, 20), (6, 21))), (33, ((6, 32), (5, 34), (5, 33), (6, 34))))}
        assert orders == {7: [1, 1, 1], 20: [1, 2, 2], 33: [1, 1, 2, 2]}, orders
    if name == "cycle":
        assert ref[0][5, 5] == 0 and ref[0][5, 6] == 0 and ref[0][5, 8] == 0 and ref[0][7, 6] == 1
    if name == "no_stream":
        assert len(ref[2]) == 0
    if name == "comb":
        assert len(ref[2]) > 400 and int(ref[2][:, 8].max()) >= 200   # a link per tributary and per stem junction; the stem's magnitude


def test_repeatable(ctx):
    i = comb()
    a, b = run_device(ctx, i, "outlets"), run_device(ctx, i, "outlets")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- refusals and plumbing ---------------------------------------------------------------------------------------------------------------------
def test_a_wrong_word_is_refused(ctx):
    i = small_inputs("y")
    with pytest.raises(ValueError):
        run_device(ctx, i, "plain", links="elsewhere")
    with pytest.raises(ValueError):
        T.streamnet(i["p"], i["src"], i["fel"], i["ad8"], links="gpu")


def test_cli_refuses_a_wrong_word_before_anything_is_read(tmp_path):
    r = subprocess.run([os.path.join(BIN, "streamnet"), "-links", "nonsense", "-p", "p.tif", "-src", "src.tif", "-fel", "fel.tif", "-ad8", "ad8.tif", "-ord",
                        str(tmp_path / "ord.tif"), "-w", str(tmp_path / "w.tif"), "-tree", str(tmp_path / "tree.txt"), "-coord", str(tmp_path / "coord.txt")],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "-links" in r.stderr and not os.listdir(tmp_path)


def test_phases_carry_the_device_builders_record(ctx):
    from taudem_amd import _lib

    i = serpentine()
    *_, ms = run_device(ctx, i, "plain", phases=True)
    assert set(ms) == set(_lib.STREAMNET_PHASES) | {"links_device"} and ms["links"] > 0
    sub = ms["links_device"]
    assert set(sub) == set(_lib.STREAMNET_LINK_PHASES) | {"jump_rounds", "level_rounds", "workspace_bytes"}
    assert sub["jump_rounds"] >= 12 and sub["level_rounds"] >= 1 and sub["workspace_bytes"] > 0
    assert sum(sub[k] for k in _lib.STREAMNET_LINK_PHASES) <= ms["links"] * 1.001 + 0.01
    *_, ms = run_device(ctx, i, "plain", links="host", phases=True)
    assert set(ms) == set(_lib.STREAMNET_PHASES)
    deep = run_device(ctx, comb(), "plain", phases=True)[-1]["links_device"]
    assert deep["level_rounds"] >= 100, deep
