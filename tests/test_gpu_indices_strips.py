"""The terrain-index tools on row strips: tdx_terrain_indices_strip, tdx_lengtharea_strip and tdx_setregion_strip on ranks of their own give the bits of the
one-device call for any cut - random cuts of two to six strips, every row a strip of its own, and for SetRegion cuts between a hole and the neighbour that
drains into it, from above and from below - and the command-line tools write the same files with --gpus 2 / 3 / 7 as with one device."""
import os
import subprocess

import numpy as np
import pytest

import indices_model as M
import taudem_amd as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")


def _in_strips(parts, nx, body):
    """body(pipe, strip) per rank, strip(x, dtype, fill) making the strip array of raster x with junk in its halo rows; the owned rows of what body returns,
    concatenated.  The halo rows of every output must still hold the mark afterwards."""
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline

    with StripGroup(len(parts), nx, [0] * len(parts)) as grp:
        def rank_main(rank, c, comm):
            y0, y1 = parts[rank]
            pipe = StripPipeline(c, comm, nx, y1 - y0)

            def strip(x, dtype, fill):
                t = pipe.empty(dtype)
                t.fill_(fill)
                if x is not None:
                    t[1:y1 - y0 + 1] = torch.from_numpy(np.ascontiguousarray(x[y0:y1])).cuda()
                return t
            outs = body(pipe, strip)
            for o in outs:
                assert np.all(torch.cat([o[0], o[-1]]).cpu().numpy() == 777), "a halo row of an output was written"
            return [o[1:y1 - y0 + 1].cpu().numpy() for o in outs]
        res = grp.run(rank_main)
    return [np.concatenate([r[k] for r in res], axis=0) for k in range(len(res[0]))]


def _all_tools(i, parts):
    """twi, sa, sar (one pass), ss and the region grid of inputs i through the strips `parts`"""
    import torch

    def body(pipe, strip):
        outs = [strip(None, torch.float32, 777.0) for _ in range(3)]
        *_, st = pipe.terrain_indices(strip(i["slp"], torch.float32, 0.5), strip(i["sca"], torch.float32, 50.0), 1.5, -0.75, out=tuple(outs))
        ss = strip(None, torch.int16, 777)
        pipe.lengtharea(strip(i["plen"], torch.float32, 3.0), strip(i["ad8"], torch.float32, 1e9), out=ss)
        reg = strip(None, torch.int32, 777)
        pipe.setregion(strip(i["p"], torch.int16, 7), strip(i["gw"], torch.int32, 1), 3, out=reg)   # a 7 in the halo row above would drain into the row below it
        return outs + [ss, reg]
    return _in_strips(parts, i["slp"].shape[1], body)


def _whole(ctx, i):
    return list(ctx.terrain_indices(i["slp"], i["sca"], 1.5, -0.75)) + [ctx.lengtharea(i["plen"], i["ad8"]), ctx.setregion(i["p"], i["gw"], 3)]


def _cuts(ny):
    from taudem_amd.distributed import partition_rows

    rng = np.random.default_rng(57 + ny)
    out = [partition_rows(ny, 2), partition_rows(ny, 3), [(0, 1), (1, ny)], [(0, ny - 1), (ny - 1, ny)], [(0, 40), (40, 41), (41, ny)]]
    for _ in range(3):
        world = int(rng.integers(2, 7))
        cuts = sorted(rng.choice(np.arange(1, ny), world - 1, replace=False).tolist())
        out.append(list(zip([0] + cuts, cuts + [ny])))
    return out


@pytest.mark.parametrize("k", range(8))
def test_strips_equal_the_whole_raster_bit_for_bit(ctx, k):
    """`holes` (96 x 100: rows of 100 cells put every strip at a start that is a multiple of four cells, of 8 bytes for int16, but not of 16 for odd rows)"""
    i = M.case_inputs("holes")
    parts = [tuple(p) for p in _cuts(i["slp"].shape[0])[k]]
    for got, want in zip(_all_tools(i, parts), _whole(ctx, i)):
        assert M.same_bits(got, want), parts


def test_every_row_a_strip_of_its_own_and_an_odd_row_length(ctx):
    i = {k: np.ascontiguousarray(v[40:48, :67]) for k, v in M.case_inputs("holes").items()}
    want = _whole(ctx, i)
    for parts in ([(y, y + 1) for y in range(8)], [(0, 5), (5, 8)]):
        for got, w in zip(_all_tools(i, parts), want):
            assert M.same_bits(got, w), parts


def test_setregion_cut_between_a_hole_and_the_neighbour_that_drains_into_it(ctx, tmp_path):
    """hole_blocks: the centres are in row 2, the neighbours k = 2, 3, 4 in row 1 (above), k = 6, 7, 8 in row 3 (below): a cut at 2 parts the centres from the
    neighbours above, a cut at 3 from those below; every row a strip of its own does both.  The restatement is the judge."""
    import torch

    restate = M.compile(tmp_path)
    p, gw = M.hole_blocks()
    want = restate.setregion(p, gw, 1)
    assert M.same_bits(ctx.setregion(p, gw, 1), want)
    centres = want[2, 2::5]
    assert centres[:8].tolist() == [1] * 8 and centres[8:11].tolist() == [int(M.MISSINGLONG)] * 3   # drained into; flows away, p == 0, p < 0
    for parts in ([(0, 2), (2, 5)], [(0, 3), (3, 5)], [(0, 2), (2, 3), (3, 5)], [(y, y + 1) for y in range(5)]):
        def body(pipe, strip):
            reg = strip(None, torch.int32, 777)
            pipe.setregion(strip(p, torch.int16, 7), strip(gw, torch.int32, 1), 1, out=reg)
            return [reg]
        assert M.same_bits(_in_strips(parts, p.shape[1], body)[0], want), parts
    p, gw = M.edge_holes()
    want = restate.setregion(p, gw, 5)
    for parts in ([(0, 1), (1, 5), (5, 6)], [(0, 3), (3, 6)]):
        def body(pipe, strip):
            reg = strip(None, torch.int32, 777)
            pipe.setregion(strip(p, torch.int16, 3), strip(gw, torch.int32, 1), 5, out=reg)
            return [reg]
        assert M.same_bits(_in_strips(parts, p.shape[1], body)[0], want), parts


@pytest.mark.parametrize("gpus", [2, 3, 7])
def test_cli_gpus_write_the_one_device_files(ctx, tmp_path, gpus):
    import test_gpu_indices as G

    i = M.case_inputs("holes")
    f = G._write(tmp_path, i)
    for tool, (args, out, banner) in G._cli_runs(f, "_1").items():
        p = subprocess.run([os.path.join(BIN, tool), *args], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, tool + p.stdout + p.stderr
        argsn, outn, _ = G._cli_runs(f, f"_{gpus}")[tool]
        p = subprocess.run([os.path.join(BIN, tool), "--gpus", str(gpus), *argsn], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and banner in p.stdout, tool + p.stdout + p.stderr
        assert open(out, "rb").read() == open(outn, "rb").read(), (tool, gpus)
    G._check_file(f, f(f"twi_{gpus}.tif"), G._expected(ctx, i)["twi"])
