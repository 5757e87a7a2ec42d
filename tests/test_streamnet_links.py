"""The product's host link builder (taudem_amd/csrc/streamnet_links.cpp) as a stand-alone program (tests/streamnet/links_main.cpp), fed the compact
stream-cell arrays the restatement dumps: its -tree and -coord files against the reference's, byte for byte.  CPU only; no HIP, nothing loaded into
the interpreter."""
import os
import subprocess

import numpy as np
import pytest

import streamnet_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "taudem_amd", "csrc")


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("streamnet_links")
    exe = os.path.join(str(d), "links_main")
    subprocess.run(["c++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", f"-I{CSRC}", os.path.join(HERE, "streamnet", "links_main.cpp"),
                    os.path.join(CSRC, "streamnet_links.cpp"), "-o", exe], check=True)
    return M.compile(d), exe, d


def run_builder(tools, tag, p, src, fel, ad8, dxc, dyc, gt, outlets, sw):
    restate, exe, d = tools
    dump = os.path.join(str(d), tag + ".bin")
    restate.run(p, src, fel, ad8, dxc, dyc, gt, *outlets, sw=sw, dump=dump)
    ny, nx = p.shape
    dxa = abs(float(np.broadcast_to(np.asarray(dxc, np.float64), (ny,))[ny // 2]))
    dya = abs(float(np.broadcast_to(np.asarray(dyc, np.float64), (ny,))[ny // 2]))
    tree, coord = os.path.join(str(d), tag + "tree.txt"), os.path.join(str(d), tag + "coord.txt")
    subprocess.run([exe, dump, str(nx), repr(dxa), repr(dya)] + [repr(float(v)) for v in gt] + [tree, coord], check=True)
    return open(tree, "rb").read(), open(coord, "rb").read()


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", M.CASES)
def test_cases_equal_reference(tools, name, variant):
    g = M.load_golden(name)
    c = M.case_fields(name)
    o = (g["cols"], g["rows"], g["ids"]) if variant == "outlets" else ((), (), ())
    tree, coord = run_builder(tools, f"{name}_{variant}", g["p"], g["src"], c["fel"], c["ad8"], c["dxc"], c["dyc"], M.gt4(g["gt"]), o, variant == "sw")
    assert tree == bytes(g["tree_" + variant]), "-tree differs"
    assert coord == bytes(g["coord_" + variant]), "-coord differs"


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", sorted(M.small_rasters()))
def test_hand_built_equal_reference(tools, name, variant):
    g = M.load_golden("small")
    p, src = M.small_rasters()[name]
    fel, ad8 = M.small_fields(p)
    o = M.SMALL_OUTLETS if variant == "outlets" else ((), (), ())
    tree, coord = run_builder(tools, f"{name}_{variant}", p, src, fel, ad8, M.SMALL_DX, M.SMALL_DY, M.gt4(M.SMALL_GT), o, variant == "sw")
    assert tree == bytes(g[f"{name}_tree_{variant}"]), "-tree differs"
    assert coord == bytes(g[f"{name}_coord_{variant}"]), "-coord differs"
