"""EditRaster on the GPU: Context.editraster and bin/editraster on the rasters and change files of tests/golden/editraster_small.npz equal the real tool's
recorded raster and what it printed; the in-place form; 67 x 5 and 300 x 70 rasters (more than one block, sizes that are no multiple of the eight cells a
lane takes) with 0, 1 and 500 changes - every corner cell, 50 duplicates, points off the raster - against the numpy model, from arrays that start on and
off a 16-byte boundary; row strips (2, 3, every row its own) with changes on every strip's first and last owned row equal the one-device result and leave
their halo rows alone; tensors stay on the device; a value no int16 holds is refused with the output untouched."""
import os
import re
import subprocess

import numpy as np
import pytest

import editraster_model as M
import taudem_amd as T
from taudem_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "taudem_amd", "bin")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "editraster_small.npz"))
CASES = M.cases()


def _changes(case, fname):
    a = GOLD[f"in/{case}"]
    x, y, v = M.scan_changes(str(GOLD[f"changes/{case}/{fname}"]))
    c, r = M.cells(x, y, M.geotransform(a.shape[0]))
    return a, int(GOLD[f"nodata/{case}"]), c, r, v


@pytest.mark.parametrize("case", list(CASES))
def test_context_equals_the_reference_raster(ctx, case):
    for fname in CASES[case][2]:
        a, nodata, c, r, v = _changes(case, fname)
        before = a.copy()
        out = ctx.editraster(a, c, r, v, nodata=nodata)
        assert out.dtype == np.int16 and np.array_equal(out, GOLD[f"out/{case}/{fname}"]), (case, fname)
        assert np.array_equal(a, before)


def _expected_stdout(case, fname):
    """The reference's words - but for what its scan of "%d" into a short does to its rank (editraster_model.process_lines): after a negative value it calls
    itself process 65535, and keeps the "Compute time" line to itself if that value was the file's last.  The project is process 0 throughout."""
    want = str(GOLD[f"stdout/{case}/{fname}"]).replace("Process: 65535 changing", "Process: 0 changing")
    return want if "Compute time: T\n" in want else want + "Compute time: T\n"


@pytest.mark.parametrize("case", list(CASES))
def test_cli_equals_the_reference_raster_and_stdout(case, tmp_path):
    a, nodata, files = CASES[case]
    T.write_raster(str(tmp_path / "in.tif"), a, int(nodata), geotransform=M.geotransform(a.shape[0]))
    for fname, text in files.items():
        (tmp_path / "changes.txt").write_text(text)
        p = subprocess.run([os.path.join(BIN, "editraster"), "-in", "in.tif", "-out", f"{fname}.tif", "-changes", "changes.txt"], capture_output=True, text=True,
                           timeout=120, cwd=tmp_path)
        assert p.returncode == 0, p.stdout + p.stderr
        assert re.sub(r"(Compute time: )[0-9.eE+-]+", r"\1T", p.stdout) == _expected_stdout(case, fname), (case, fname)
        assert p.stderr == "Time estimate not available.\n"
        out, info = T.read_raster(str(tmp_path / f"{fname}.tif"), np.int16)
        assert float(info["nodata"]) == -32768.0 and np.array_equal(out, GOLD[f"out/{case}/{fname}"]), (case, fname)
    if a.shape[0] >= 3:   # the same bytes from three strips
        p = subprocess.run([os.path.join(BIN, "editraster"), "--gpus", "3", "-in", "in.tif", "-out", "three.tif", "-changes", "changes.txt"], capture_output=True,
                           text=True, timeout=120, cwd=tmp_path)
        assert p.returncode == 0, p.stdout + p.stderr
        assert (tmp_path / "three.tif").read_bytes() == (tmp_path / f"{fname}.tif").read_bytes()


def test_gpu_runs_reproduce_the_recorded_transcripts():
    """bin/editraster on one GPU and on three rank threads: status, stdout, stderr and the SHA-256 of the raster of tests/golden/tool_transcripts_editraster.json"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("editraster_transcripts", os.path.join(ROOT, "scripts", "editraster_transcripts.py"))
    et = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(et)
    expected = et.load_fixture(os.path.join(ROOT, "tests", "golden", "tool_transcripts_editraster.json"), "gpu")
    assert len(expected) == 4 and all(e["status"] == 0 and e["files"]["out.tif"] for e in expected.values())
    for name in ("edges", "dup"):
        assert expected[f"gpu1/wide/editraster/{name}"]["files"] == expected[f"gpu3/wide/editraster/{name}"]["files"]
    bad = et.differences(expected, et.collect("gpu"))
    assert not bad, "\n".join(bad)


def _random_case(ny, nx, n, seed):
    """a raster with nodata runs, and n changes: the four corners first (when n allows), then random cells of which some lie off the raster, and among 500 changes
    50 that repeat an earlier cell with another value"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-5, 40, size=(ny, nx)).astype(np.int16)   # nodata is 3: a tenth of a percent would not meet every lane position
    c = rng.integers(-3, nx + 3, n)
    r = rng.integers(-3, ny + 3, n)
    v = rng.integers(-32768, 32768, n)
    corners = [(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)]
    for k, (cc, rr) in enumerate(corners[:n]):
        c[k], r[k] = cc, rr
    if n >= 500:
        src = rng.integers(0, n - 50, 50)
        c[n - 50:], r[n - 50:] = c[src], r[src]
        assert len({(int(x), int(y)) for x, y in zip(c, r)}) <= n - 50
    return a, c, r, v


@pytest.mark.parametrize("shape", [(5, 67), (70, 300)])
@pytest.mark.parametrize("n", [0, 1, 500])
def test_equals_the_numpy_model(ctx, shape, n):
    import torch

    a, c, r, v = _random_case(*shape, n, 1000 + n + shape[1])
    want = M.edit(a, 3, c, r, v)
    assert np.array_equal(ctx.editraster(a, c, r, v, nodata=3), want)
    # tensors: the result is a tensor on the input's device, the input is not written; arrays that start 2 bytes past a 16-byte boundary take element accesses
    t = torch.from_numpy(a).cuda()
    o = ctx.editraster(t, c, r, v, nodata=3)
    assert o.is_cuda and o.device == t.device and o.dtype == torch.int16 and o.data_ptr() != t.data_ptr()
    assert np.array_equal(o.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), a)
    cells = a.size
    for shift_in, shift_out in ((1, 0), (0, 1), (1, 1), (4, 4)):
        big_in = torch.full((cells + 8,), 555, dtype=torch.int16, device="cuda")
        big_out = torch.full((cells + 8,), 777, dtype=torch.int16, device="cuda")
        ti = big_in[shift_in:shift_in + cells].view(shape)
        ti.copy_(t)
        to = big_out[shift_out:shift_out + cells].view(shape)
        assert ctx.editraster(ti, c, r, v, nodata=3, out=to) is to
        assert np.array_equal(to.cpu().numpy(), want), (shift_in, shift_out)
        rest = torch.cat([big_out[:shift_out], big_out[shift_out + cells:]]).cpu().numpy()
        assert np.all(rest == 777), "cells beside the output were written"


def test_in_place(ctx):
    import torch

    a, c, r, v = _random_case(70, 300, 500, 77)
    want = M.edit(a, 3, c, r, v)
    t = torch.from_numpy(a).cuda()
    ptr = t.data_ptr()
    assert ctx.editraster(t, c, r, v, nodata=3, out=t) is t and t.data_ptr() == ptr
    assert np.array_equal(t.cpu().numpy(), want)
    b = a.copy()
    assert ctx.editraster(b, c, r, v, nodata=3, out=b) is b and np.array_equal(b, want)
    # a second pass over the result changes nothing but the cells whose new value was the old nodata value
    again = ctx.editraster(t, c, r, v, nodata=3, out=t).cpu().numpy()
    assert np.array_equal(again, M.edit(want, 3, c, r, v))


def test_a_value_outside_int16_is_refused_and_nothing_is_written(ctx):
    import torch

    a = np.arange(12, dtype=np.int16).reshape(3, 4)
    for vals in ([5, 32768], [-32769, 5], [2 ** 40, 1]):
        for make in (lambda x: x, lambda x: torch.from_numpy(x).cuda()):
            out = make(np.full((3, 4), 777, np.int16))
            with pytest.raises(_lib.TdxError) as e:
                ctx.editraster(make(a), [0, 99], [0, 99], vals, out=out)   # the second cell lies off the raster: its value is judged all the same
            assert e.value.code == _lib.TDX_ERR_ARG and "outside -32768 .. 32767" in str(e.value)
            assert np.all((out.cpu().numpy() if hasattr(out, "cpu") else out) == 777)
    with pytest.raises(ValueError):
        ctx.editraster(a, [0, 1], [0], [1, 2])


def _in_strips(parts, a, c, r, v, nodata, in_place):
    import torch

    from taudem_amd.distributed import StripGroup, StripPipeline

    nx = a.shape[1]
    with StripGroup(len(parts), nx, [0] * len(parts)) as grp:
        def rank_main(rank, cx, comm):
            y0, y1 = parts[rank]
            pipe = StripPipeline(cx, comm, nx, y1 - y0)
            t = pipe.empty(torch.int16)
            t.fill_(nodata)   # a halo row of nodata cells: recoded to -32768 if the pass touched it
            t[1:y1 - y0 + 1] = torch.from_numpy(np.ascontiguousarray(a[y0:y1])).cuda()
            if in_place:
                o = pipe.editraster(t, c, r, v, y0, out=t, nodata=nodata)[0]
                assert o is t
                halo = nodata
            else:
                o = pipe.empty(torch.int16)
                o.fill_(777)
                assert pipe.editraster(t, c, r, v, y0, out=o, nodata=nodata)[0] is o
                halo = 777
            assert np.all(torch.cat([o[0], o[-1]]).cpu().numpy() == halo), "a halo row of the output was written"
            return o[1:y1 - y0 + 1].cpu().numpy()
        return np.concatenate(grp.run(rank_main), axis=0)


@pytest.mark.parametrize("shape,cuts", [((5, 67), "rows"), ((5, 67), 2), ((70, 300), 2), ((70, 300), 3), ((11, 72), 3), ((11, 72), "rows")])
def test_strips_equal_the_whole_raster(ctx, shape, cuts):
    """(rows of 72 cells put every strip on a 16-byte boundary, rows of 67 and 300 cells do not)"""
    from taudem_amd.distributed import partition_rows

    ny, nx = shape
    parts = [(y, y + 1) for y in range(ny)] if cuts == "rows" else [tuple(p) for p in partition_rows(ny, cuts)]
    a, c, r, v = _random_case(ny, nx, 500, 31 + nx)
    edge_rows = sorted({y for p in parts for y in (p[0], p[1] - 1)})
    ec = np.array([0, nx - 1, nx // 2] * len(edge_rows))
    er = np.repeat(edge_rows, 3)
    c, r, v = np.concatenate([c, ec, ec[:3]]), np.concatenate([r, er, er[:3]]), np.concatenate([v, np.arange(len(ec)) + 100, [-1, -2, -3]])
    want = ctx.editraster(a, c, r, v, nodata=3)
    assert np.array_equal(want, M.edit(a, 3, c, r, v)) and want[edge_rows[-1], nx - 1] == 100 + len(ec) - 2 and want[edge_rows[0], 0] == -1
    for in_place in (False, True):
        assert np.array_equal(_in_strips(parts, a, c, r, v, 3, in_place), want), (parts, in_place)
