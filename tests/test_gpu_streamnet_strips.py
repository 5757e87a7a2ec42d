"""StreamNet in row strips (StripPipeline.streamnet_compact -> StreamNetLinks -> StripPipeline.streamnet_label): the same rasters as
tests/test_gpu_streamnet.py under arbitrary cuts - random cuts of two to six strips, strips of a single row, and cuts that run along a stream (between
the two horizontal streams of the hand-built `off_each_edge`, and on both sides of the stream row led off the west edge in every case) - must give the
bytes of the one-device result: the goldens' -ord, -w, -tree and -coord where there is a golden, Context.streamnet's otherwise.  All ranks share one GPU
(the library's in-process rank group); the sweeps run under the verifier."""
import numpy as np
import pytest

import streamnet_model as M
from test_gpu_streamnet import assert_files_equal_golden, case_inputs, generated, run_cli, run_context, small_inputs

pytestmark = pytest.mark.gpu


def random_cuts(ny, seed, world=None):
    """[(y0, y1)]: `world` strips (2..6 by default) with cut rows drawn at random, so strips of one row come up"""
    rng = np.random.default_rng(seed)
    world = min(ny, world or int(rng.integers(2, 7)))
    rows = np.sort(rng.choice(np.arange(1, ny), world - 1, replace=False)) if world > 1 else np.zeros(0, np.int64)
    edges = [0, *[int(r) for r in rows], ny]
    return list(zip(edges[:-1], edges[1:]))


def in_strips(i, parts, variant):
    """(ord, w, tree, coord) of the strips put together"""
    import torch

    from taudem_amd import StreamNetLinks
    from taudem_amd.distributed import StripGroup, StripPipeline, strip_rows

    ny, nx = i["p"].shape
    world = len(parts)
    dx = np.broadcast_to(np.asarray(i["dx"], np.float64), (ny,))
    dy = np.broadcast_to(np.asarray(i["dy"], np.float64), (ny,))
    state = [None] * world
    with StripGroup(world, nx, [0] * world) as grp:
        def compact(r, c, comm):
            y0, y1 = parts[r]
            pipe = StripPipeline(c, comm, nx, y1 - y0)

            def put(a):
                t = pipe.empty(getattr(torch, np.asarray(a).dtype.name))
                t[1:y1 - y0 + 1] = torch.from_numpy(np.ascontiguousarray(a[y0:y1])).cuda()
                return t
            p, src = put(i["p"]), put(i["src"])
            part, _ = pipe.streamnet_compact(p, src, put(i["fel"]), put(i["ad8"]), y0, strip_rows(dx, y0, y1), strip_rows(dy, y0, y1))
            state[r] = (pipe, p, src)
            return part
        handles = grp.run(compact)
        with StreamNetLinks(handles, nx, ny, dx, dy, i["gt"], i["outlets"] if variant == "outlets" else None) as links:
            def label(r, c, comm):
                pipe, p, src = state[r]
                ordg, w, _ = pipe.streamnet_label(p, src, links.parts[r], links.handle, links.first_cell[r], variant == "sw")
                return ordg[1:-1].cpu().numpy(), w[1:-1].cpu().numpy()
            res = grp.run(label)
            tree, coord = links.tree, links.coord
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res]), tree, coord


def stream_row_cuts(i):
    """cuts on both sides of the longest horizontal run of stream cells"""
    ny = i["p"].shape[0]
    stream = (i["src"] > 0) & (i["p"] != M.P_NODATA)
    y = int(np.argmax(((stream[:, :-1] & stream[:, 1:]) & np.isin(i["p"][:, :-1], (1, 5))).sum(axis=1)))
    edges = sorted({0, y, y + 1, ny})
    return list(zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("variant", M.VARIANTS)
@pytest.mark.parametrize("name", M.CASES)
def test_cases_under_random_cuts(monkeypatch, name, variant):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    g, i = case_inputs(name)
    parts = random_cuts(i["p"].shape[0], 41 + M.CASES.index(name) * 3 + M.VARIANTS.index(variant))
    M.assert_equals_golden(f"{name}/{variant} in strips {parts}", in_strips(i, parts, variant), g, variant)


@pytest.mark.parametrize("name", M.CASES)
def test_cases_cut_along_a_stream(monkeypatch, name):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    g, i = case_inputs(name)
    parts = stream_row_cuts(i)
    assert any(y1 - y0 == 1 for y0, y1 in parts), parts
    M.assert_equals_golden(f"{name}/outlets in strips {parts}", in_strips(i, parts, "outlets"), g, "outlets")


@pytest.mark.parametrize("name", sorted(M.small_rasters()))
def test_hand_built_in_one_row_strips(name):
    """every row a strip of its own: both halo rows of a strip are the only owned row of a neighbour"""
    g = M.load_golden("small")
    i = small_inputs(name)
    ny = i["p"].shape[0]
    parts = [(y, y + 1) for y in range(ny)]
    for variant in ("outlets", "sw"):
        M.assert_equals_golden(f"{name}/{variant} in {ny} one-row strips", in_strips(i, parts, variant), g, variant, name + "_")


def test_hand_built_cut_between_two_streams():
    g = M.load_golden("small")
    i = small_inputs("off_each_edge")   # horizontal streams on rows 4 and 5
    M.assert_equals_golden("off_each_edge cut at row 5", in_strips(i, [(0, 5), (5, 9)], "plain"), g, "plain", "off_each_edge_")


@pytest.mark.parametrize("shape,seed", [((65, 129), 0), ((130, 150), 1), ((130, 150), 2)])
def test_generated_rasters_equal_one_device(ctx, oracle, monkeypatch, shape, seed):
    monkeypatch.setenv("TDX_SWEEP_VERIFY", "1")
    i = generated(ctx, oracle, shape, 11 + shape[0])
    parts = random_cuts(shape[0], 7 + seed, world=None if seed else 4)
    for variant in ("outlets", "sw"):
        one = run_context(ctx, i, variant)
        got = in_strips(i, parts, variant)
        what = f"{shape} {variant} in strips {parts}"
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]), f"{what}: {int(np.sum(got[0] != one[0]))} order cells, {int(np.sum(got[1] != one[1]))} labels differ"
        assert np.array_equal(got[2], one[2]) and np.array_equal(got[3].view(np.uint64), one[3].view(np.uint64)), f"{what}: link rows differ"


@pytest.mark.parametrize("name,variant,gpus", [("holes", "outlets", 3), ("geographic", "plain", 2), ("rect_dxdy", "sw", 7)])
def test_cli_with_gpus(tmp_path, name, variant, gpus):
    """bin/streamnet --gpus N: N rank threads (on this one GPU), the reference's equal strips, the same four files"""
    g, i = case_inputs(name)
    got = run_cli(tmp_path, i, variant, gpus=gpus)
    assert_files_equal_golden(f"{name}/{variant} --gpus {gpus}", got, g, variant)
    assert f"Processors: {gpus}\nRead time: " in got[4].stdout


def test_cli_with_more_gpus_than_rows(tmp_path):
    g = M.load_golden("small")
    got = run_cli(tmp_path, small_inputs("y"), "outlets", gpus=16)   # 9 rows: nine one-row ranks
    assert_files_equal_golden("y --gpus 16", got, g, "outlets", "y_")
    assert "Processors: 9\n" in got[4].stdout
