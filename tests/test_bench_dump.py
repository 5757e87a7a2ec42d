"""bench.py --dump-outputs DIR: what the last timed step returned, as float32 .npy files within 64 MB in all (bench.dump_outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, bits_equal, describe_diff


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_full_and_sampled(tmp_path, monkeypatch):
    """CPU: small rasters are written whole; beyond the budget every raster is reduced to the same seeded sample of cells, listed in
    sample_index.npy, the same from call to call; with ranks each rank writes its own files within its share of the budget."""
    import torch

    import bench

    assert bench.DUMP_SAMPLE_CELLS * (4 * 4 + 8) <= bench.DUMP_MAX_BYTES     # the four D8 rasters and the index of a sample fit
    g = torch.Generator().manual_seed(3)
    x = torch.rand((1000, 700), generator=g)
    p = (torch.rand((1000, 700), generator=g) * 9).to(torch.int16)

    bench.dump_outputs(torch, str(tmp_path / "full"), {"x": x, "p": p})
    assert sorted(os.listdir(tmp_path / "full")) == ["p.npy", "x.npy"]
    assert bits_equal(np.load(tmp_path / "full" / "x.npy"), x.numpy())
    pf = np.load(tmp_path / "full" / "p.npy")
    assert pf.dtype == np.float32 and np.array_equal(pf, p.numpy().astype(np.float32))

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 20)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_CELLS", 1 << 15)
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), {"x": x, "p": p})
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == ["p.npy", "sample_index.npy", "x.npy"] and _sizes(a) <= 1 << 20
    idx = np.load(a / "sample_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 1 << 15 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < x.numel()
    k = idx.astype(np.int64)
    assert bits_equal(np.load(a / "x.npy"), x.numpy().reshape(-1)[k])
    assert np.array_equal(np.load(a / "p.npy"), p.numpy().reshape(-1)[k].astype(np.float32))
    for f in os.listdir(a):
        assert bits_equal(np.load(a / f), np.load(b / f)), f

    for r in range(4):
        bench.dump_outputs(torch, str(tmp_path / "ranks"), {"x": x, "p": p}, r, 4)
    assert sorted(os.listdir(tmp_path / "ranks")) == sorted(f"{n}.rank{r}.npy" for n in ("p", "sample_index", "x") for r in range(4))
    assert _sizes(tmp_path / "ranks") <= 1 << 20


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_pipeline_outputs(tmp_path, oracle):
    """`bench.py --dump-outputs DIR` on a small raster: fel, p, sd8 and ad8 of the timed path, identical in two runs with the same arguments and
    bit-exact against the restatement on the same seeded DEM."""
    n, seed = 384, 1234
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--size", str(n), "--seed", str(seed), "--steps", "2", "--warmup", "1",
                            "--cpu-sample", "0", "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert lines[0]["steps"] == 2 and lines[0]["ms_per_step"] > 0
    names = ["ad8.npy", "fel.npy", "p.npy", "sd8.npy"]
    assert sorted(os.listdir(tmp_path / "a")) == names and sorted(os.listdir(tmp_path / "b")) == names
    got = {}
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and a.shape == (n, n), (f, a.dtype, a.shape)
        assert bits_equal(a, b), describe_diff(a, b, f + " run to run")
        got[f[:-4]] = a
    fel = oracle.pitremove(oracle.synth_dem(n, seed), -9999.0)
    p, sd8, _ = oracle.d8flowdir(fel, -3.0e38, 30.0, 30.0)
    ad8 = oracle.aread8(p, -32768)
    for name, want in (("fel", fel), ("p", p.astype(np.float32)), ("sd8", sd8), ("ad8", ad8)):
        assert bits_equal(got[name], want), describe_diff(got[name], want, name)
