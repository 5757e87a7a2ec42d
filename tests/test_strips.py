"""Row strips across ranks (taudem_amd/distributed.py): protocol tests on CPU (gloo, world size 2 and 3)
and, on the GPU box, full PitRemove -> D8FlowDir -> AreaD8 runs with 2-4 ranks sharing the GPU, compared
bit-for-bit with the CPU oracle by tests/strip_worker.py."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "strip_worker.py")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(nproc, extra, timeout=600):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), WORKER] + extra
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OMP_NUM_THREADS"] = "1"
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{' '.join(cmd)}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-6000:]}"
    return r.stdout


def test_partition_rows_matches_linearpart():
    from taudem_amd.distributed import partition_rows

    assert partition_rows(10, 3) == [(0, 3), (3, 6), (6, 10)]      # remainder to the last rank (src/linearpart.h:133-134)
    assert partition_rows(8, 1) == [(0, 8)]
    assert partition_rows(65536, 8)[3] == (3 * 8192, 4 * 8192)


def test_strip_rows_takes_the_neighbouring_global_rows_as_halo():
    """Per-row values of a strip: its own rows plus the global rows y0 - 1 and y1 as halo rows, clamped into the raster (rows_of in
    taudem_amd/csrc/tool_strips.hpp) - the geometry the 1-rank reference gives a strip's edge cells.  Scalars pass through."""
    import numpy as np

    from taudem_amd.distributed import partition_rows, strip_rows

    g = np.arange(10, dtype=np.float64) * 1.5 + 7.0
    assert strip_rows(g, 0, 3).tolist() == [g[0], g[0], g[1], g[2], g[3]]
    assert strip_rows(g, 3, 6).tolist() == [g[2], g[3], g[4], g[5], g[6]]
    assert strip_rows(g, 6, 10).tolist() == [g[5], g[6], g[7], g[8], g[9], g[9]]
    assert strip_rows(g, 0, 10).tolist() == [g[0], *g.tolist(), g[9]]
    assert strip_rows(g, 4, 5).tolist() == [g[3], g[4], g[5]]
    for y0, y1 in partition_rows(10, 3):
        assert strip_rows(g, y0, y1)[1:-1].tolist() == g[y0:y1].tolist()
    assert strip_rows(30.0, 2, 5) == 30.0
    with pytest.raises(ValueError):
        strip_rows(g, 8, 11)


@pytest.mark.parametrize("nproc", [2, 3])
def test_stripcomm_protocol_gloo(nproc):
    _launch(nproc, ["--protocol"], timeout=300)


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,case", [(2, "plain"), (3, "short_strips"), (2, "holes"), (4, "big"), (1, "plain"), (4, "wide"), (2, "plain+dinf"), (3, "holes+dinf"), (4, "short_strips+dinf"),
                                       (3, "geographic+dinf")])
def test_strips_bit_exact_vs_oracle(nproc, case):
    out = _launch(nproc, ["--case", case], timeout=900)
    assert f"{nproc} ranks bit-exact vs oracle" in out
