"""The model of ad8_tile_fast_kernel's pointer-doubling schedule (scripts/sim/ad8_doubling.c) on a small raster of the restatement's directions: it must build, the
counts of every clean tile must equal the counts made by walking every cell's path, no tile may need more than 12 rounds, and a 2-cycle planted in a clean tile must
leave a pointer live after the 12th round (docs/experiments_r07.md section 1)."""
import os
import re
import subprocess

import numpy as np
import pytest

N = 256


@pytest.fixture(scope="module")
def model(tmp_path_factory, oracle):
    tmp = tmp_path_factory.mktemp("ad8_doubling")
    exe = tmp / "ad8_doubling"
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "sim", "ad8_doubling.c")
    subprocess.run(["gcc", "-O2", "-w", "-o", str(exe), src], check=True)
    dem = oracle.synth_dem((N, N), 1234)
    fel = oracle.pitremove(dem, -9999.0)
    p, _, _ = oracle.d8flowdir(fel, -3.0e38, 30.0, 30.0)

    def run(p, name):
        raw = tmp / name
        np.ascontiguousarray(p, dtype=np.int16).tofile(raw)
        out = subprocess.run([str(exe), str(p.shape[0]), str(raw)], check=True, capture_output=True, text=True).stdout
        m = re.search(r"tiles (\d+): clean (\d+), cyclic (\d+), mismatching (\d+); rounds per tile ([\d.]+), at most (\d+)", out)
        assert m, out
        live = [int(v) for v in re.search(r"live cells per round:((?: \d+)+)", out)[1].split()]
        return {"tiles": int(m[1]), "clean": int(m[2]), "cyclic": int(m[3]), "mismatching": int(m[4]), "rounds": float(m[5]), "max_rounds": int(m[6]), "live": live}
    return p, run


def _clean_tiles(p):
    """Tiles whose 66 x 66 window lies inside the raster and holds codes 1 .. 8 only."""
    n, count = p.shape[0], 0
    for ty in range(1, n // 64 - 1):
        for tx in range(1, n // 64 - 1):
            w = p[ty * 64 - 1:ty * 64 + 65, tx * 64 - 1:tx * 64 + 65]
            count += bool(((w >= 1) & (w <= 8)).all())
    return count


def test_clean_tiles_reproduce_the_direct_counts(model):
    p, run = model
    r = run(p, "p.bin")
    assert r["tiles"] == (N // 64) ** 2
    assert r["clean"] == _clean_tiles(p) > 0 and r["cyclic"] == 0
    assert r["mismatching"] == 0
    assert 1 <= r["max_rounds"] <= 12
    assert r["live"][0] <= 4096 and all(a >= b for a, b in zip(r["live"], r["live"][1:])), "a dead pointer stays dead"
    assert all(v == 0 for v in r["live"][r["max_rounds"]:])


def test_a_planted_cycle_is_still_live_after_twelve_rounds(model):
    p, run = model
    base = run(p, "p.bin")
    assert _clean_tiles(p) == base["clean"] >= 1
    # a 2-cycle in the middle of a tile the model found clean
    q = p.copy()
    ty, tx = next((ty, tx) for ty in range(1, N // 64 - 1) for tx in range(1, N // 64 - 1)
                  if ((p[ty * 64 - 1:ty * 64 + 65, tx * 64 - 1:tx * 64 + 65] >= 1) & (p[ty * 64 - 1:ty * 64 + 65, tx * 64 - 1:tx * 64 + 65] <= 8)).all())
    y, x = ty * 64 + 30, tx * 64 + 30
    q[y, x] = 1
    q[y, x + 1] = 5
    r = run(q, "q.bin")
    assert r["cyclic"] == 1 and r["clean"] == base["clean"] - 1
    assert r["mismatching"] == 0


def test_the_longest_possible_path_needs_exactly_twelve_rounds(model):
    _, run = model
    p = np.full((192, 192), 1, dtype=np.int16)          # everything flows east ...
    for ly in range(64):                                 # ... but the centre tile is one boustrophedon path through all its 4096 cells, leaving south
        row = 64 + ly
        p[row, 64:128] = 1 if ly % 2 == 0 else 5
        p[row, 127 if ly % 2 == 0 else 64] = 7
    r = run(p, "snake.bin")
    assert r["clean"] == 1 and r["cyclic"] == 0 and r["mismatching"] == 0
    assert r["max_rounds"] == 12
