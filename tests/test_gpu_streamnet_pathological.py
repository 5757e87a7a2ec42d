"""StreamNet on inputs that are nothing like a fractal surface (tests/pathological.py): planes, ramps, a spiral, single rows and columns, rasters without
data, NaN and Inf cells.  fel, p and ad8 are the CPU oracle's; src = 1 where ad8 reaches a fiftieth of its largest value (at least 4), nodata where ad8
is.  The expected values are the serial restatement's (tests/streamnet_model.py, which tests/test_streamnet_restatement.py holds to the reference): it
finishes on all 18 rasters.  Rasters, tree rows and coord rows are compared exactly - the coord rows as bit patterns, because fel may be NaN or
infinite there.  Each case runs under the sweep verifier, without outlets, with outlets and with -sw."""
import numpy as np
import pytest

import pathological as PG
import streamnet_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("streamnet"))


def patho_case(oracle, name):
    dem = np.ascontiguousarray(PG.CASES[name](oracle), np.float32)
    fel = oracle.pitremove(dem, PG.NODATA)
    p, _, _ = oracle.d8flowdir(fel, -3.0e38, 30.0, 30.0)
    ad8 = oracle.aread8(p, -32768, contcheck=False)
    src = np.where(ad8 >= max(4.0, float(ad8.max()) / 50.0), 1, 0).astype(np.int32)
    src[ad8 < -0.5] = M.SRC_NODATA
    ny, nx = p.shape
    on = np.flatnonzero((src == 1) & (p != M.P_NODATA))
    picks = on[:: max(1, on.size // 5)][:5] if on.size else np.zeros(0, np.int64)
    outlets = (np.append(picks % nx, nx + 1).astype(np.int32), np.append(picks // nx, 0).astype(np.int32), np.arange(10, 10 + picks.size + 1, dtype=np.int32))
    return dict(p=p, src=src, fel=fel, ad8=ad8, outlets=outlets)


@pytest.mark.parametrize("name", sorted(PG.CASES))
def test_one_device_on_pathological_input(ctx, oracle, restate, monkeypatch, name):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    c = patho_case(oracle, name)
    gt = (100.0, 30.0, 0.0, 9000.0, 0.0, -30.0)
    for variant in M.VARIANTS:
        o = c["outlets"] if variant == "outlets" else None
        ref = restate.run(c["p"], c["src"], c["fel"], c["ad8"], 30.0, 30.0, M.gt4(gt), *(o or ((), (), ())), sw=variant == "sw")
        ordg, w, tree, coord = ctx.streamnet(c["p"], c["src"], c["fel"], c["ad8"], o, variant == "sw", dx=30.0, dy=30.0, geotransform=gt)
        tag = f"{name}/{variant}"
        assert np.array_equal(ordg, ref[0]), f"{tag}: {int(np.sum(ordg != ref[0]))} order cells differ"
        assert np.array_equal(w, ref[1]), f"{tag}: {int(np.sum(w != ref[1]))} labels differ"
        assert np.array_equal(tree, ref[2]), f"{tag}: tree rows differ"
        assert coord.shape == ref[3].shape and np.array_equal(coord.view(np.uint64), ref[3].view(np.uint64)), f"{tag}: coord rows differ"
