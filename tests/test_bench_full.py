"""bench.py --full: a plain run times its steps and prints its line; the roofline pass, the CPU baseline and the other configurations' legs
come with --full only."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def test_full_is_off_by_default(monkeypatch):
    """CPU: --full is an option of every run, off unless given; --cpu-sample / --no-extras keep their defaults."""
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.cpu_sample == 2048 and a.no_extras is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--cpu-sample", "0"])
    a = bench.parse()
    assert a.full is True and a.cpu_sample == 0


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_line_and_full_line():
    """A plain run on a small raster carries the headline fields and the timed steps' own figures, but no roofline and no CPU baseline;
    the same run with --full adds both and leaves the headline fields' meaning as it is."""
    common = ["--size", "256", "--steps", "2", "--warmup", "1"]
    plain = _bench(common)
    full = _bench(common + ["--full", "--cpu-sample", "128"])
    for line in (plain, full):
        assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert "stage_ms_per_step" in line and "roofline_streaming_stencil" in line
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "config"):
        assert plain[k] == full[k], k
    assert "roofline" not in plain and "cpu_baseline" not in plain
    assert full["roofline"]["launches_per_step"] >= 1 and full["roofline"]["avg_launch_ms"] > 0
    assert full["cpu_baseline"]["value"] > 0
