"""The C++ restatement of StreamNet (tests/streamnet_model.py) against the reference's one-rank outputs (tests/golden/streamnet_*.npz): the -ord
and -w rasters exactly, the -tree and -coord files byte for byte, for the five cases and the hand-built rasters, each without outlets, with outlets
and with -sw.  CPU only."""
import numpy as np
import pytest

import streamnet_model as M


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("streamnet"))


def check(tag, got, g, variant, prefix=""):
    M.assert_equals_golden(tag, got, g, variant, prefix)


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", M.CASES)
def test_cases_equal_reference(restate, name, variant):
    g = M.load_golden(name)
    c = M.case_fields(name)
    o = (g["cols"], g["rows"], g["ids"]) if variant == "outlets" else ((), (), ())
    got = restate.run(g["p"], g["src"], c["fel"], c["ad8"], c["dxc"], c["dyc"], M.gt4(g["gt"]), *o, sw=variant == "sw")
    check(f"{name}/{variant}", got, g, variant)


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", sorted(M.small_rasters()))
def test_hand_built_equal_reference(restate, name, variant):
    g = M.load_golden("small")
    assert name in set(g["names"].tolist()), f"the reference did not finish on {name}"
    p, src = M.small_rasters()[name]
    fel, ad8 = M.small_fields(p)
    o = M.SMALL_OUTLETS if variant == "outlets" else ((), (), ())
    got = restate.run(p, src, fel, ad8, M.SMALL_DX, M.SMALL_DY, M.gt4(M.SMALL_GT), *o, sw=variant == "sw")
    check(f"{name}/{variant}", got, g, variant, name + "_")


def test_goldens_cover_the_quirks():
    """At least 20 links per case; a junction of three or more inflows, a stream off the raster's edge and a src cell of value 2 somewhere; outlets on a
    junction, mid-link, on a source, off the stream, off the raster and two on one cell in every case."""
    k3 = edge = two = False
    for name in M.CASES:
        g = M.load_golden(name)
        p, src = g["p"], g["src"]
        nx = p.shape[1]
        stream, recv, nin = M.stream_graph(p, src)
        assert bytes(g["tree_plain"]).count(b"\n") >= 20, name
        k3 |= bool(np.any(nin[stream.ravel()] >= 3))
        edge |= bool(np.any(stream.ravel() & (recv < 0) & (p.ravel() > 0)))
        two |= bool(np.any(src == 2))
        oc = g["rows"][:6].astype(np.int64) * nx + g["cols"][:6]
        assert nin[oc[0]] >= 2 and nin[oc[1]] == 1 and nin[oc[2]] == 0 and stream.flat[oc[2]] and not stream.flat[oc[3]] and oc[4] == oc[5], name
        assert not 0 <= g["cols"][6] < nx, name
        assert not np.array_equal(g["w_plain"], g["w_outlets"]) and set(np.unique(g["w_sw"]).tolist()) == {M.W_NODATA, 1}, name
    assert k3 and edge and two
    assert len(M.load_golden("small")["names"]) >= len(M.small_rasters()) - 2
