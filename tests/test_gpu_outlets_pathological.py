"""MoveOutletsToStrm and ConnectDown on inputs that are nothing like a fractal surface (tests/pathological.py): planes, ramps, a spiral, single rows
and columns, rasters without data, NaN and Inf cells.  p, src and ad8 are those of tests/test_gpu_streamnet_pathological.py, w is StreamNet's
watershed grid of them.  The expected values are the serial restatement's (tests/outlets_model.py, which tests/test_outlets_restatement.py holds to
the reference).  Outlets on every 53rd cell and a few off the raster; ConnectDown also with fel in the place of ad8, which brings NaN and infinite
values into the arg-max."""
import numpy as np
import pytest

import outlets_model as M
import pathological as PG
from test_gpu_streamnet_pathological import patho_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("outlets"))


@pytest.mark.parametrize("name", sorted(PG.CASES))
def test_one_device_on_pathological_input(ctx, oracle, restate, name):
    c = patho_case(oracle, name)
    p, src = c["p"], c["src"]
    ny, nx = p.shape
    _, w, _, _ = ctx.streamnet(p, src, c["fel"], c["ad8"], dx=30.0, dy=30.0)
    cells = np.arange(0, p.size, 53)
    cols, rows = np.append(cells % nx, [-1, nx, 0]).astype(np.int32), np.append(cells // nx, [0, 0, ny]).astype(np.int32)
    for md in (50, 2):
        want = restate.moveoutlets(p, src, cols, rows, md)
        got = ctx.moveoutletstostrm(p, src, (cols, rows), md, src_nodata=M.SRC_NODATA)
        assert all(np.array_equal(a, b) for a, b in zip(want, got)), f"{name}: -md {md}"
    for field in ("ad8", "fel"):
        for dd in (10, 1):
            want = restate.connectdown(p, w, c[field], dd)
            got = ctx.connectdown(p, w, c[field], dd)
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(want, got)), f"{name}: {field} -d {dd}"
