"""Id grids for the ring builders beyond those of tests/test_gpu_polygonize.py: the shapes at which the device ring builder
(taudem_amd/csrc/polygon_rings_device.hip) can go wrong.  Shared by its model's test, which runs without a GPU, and by its GPU test."""
import numpy as np

from polygonize_model import NODATA as ND


def _serpentine():
    """96 x 128: a one-cell-wide serpentine of id 7 over the columns 0 .. 99 (one ring of about 9.7 k edges, between the jump rounds 2^13 and 2^14)
    beside 500 single cells of id 3 (500 rings of four edges, one feature)."""
    w = np.full((96, 128), ND, np.int32)
    for k, r in enumerate(range(0, 96, 2)):
        w[r, 0:100] = 7
        if r + 1 < 95:
            w[r + 1, 99 if k % 2 == 0 else 0] = 7
    n = 0
    for r in range(0, 96, 2):
        for c in range(102, 128, 2):
            if n < 500:
                w[r, c] = 3
                n += 1
    assert n == 500
    return w


def _stack(n):
    w = np.full((2 * n + 2, 5), 1, np.int32)
    w[1:2 * n:2, 2] = ND
    return w


def _side_by_side():
    w = np.full((5, 7), 1, np.int32)
    w[1, 1] = ND   # above the left one of the two holes below: its walk ends on this hole, the right one's on the outer ring
    w[3, 1] = ND
    w[3, 4] = ND
    return w


def _bottom_hole():
    w = np.full((300, 8), 1, np.int32)
    w[298, 3] = ND   # 298 rows up to the outer ring: five strides of 64 rows
    return w


def _hole_island_hole():
    w = np.full((9, 9), 1, np.int32)
    w[1:8, 1:8] = 2
    w[2:7, 2:7] = 1
    w[3:6, 3:6] = 2
    w[4, 4] = ND
    return w


CASES = {
    "serpentine_96x128": _serpentine(),
    "holes_stacked_3": _stack(3),
    "holes_stacked_5": _stack(5),
    "holes_side_by_side": _side_by_side(),
    "hole_bottom_300x8": _bottom_hole(),
    "hole_island_hole": _hole_island_hole(),
}


def random_grid(seed):
    """Sides 3 .. 40 by 3 .. 70, two to four ids, 0 - 30 % nodata."""
    rng = np.random.default_rng(1000 + seed)
    ny, nx = int(rng.integers(3, 41)), int(rng.integers(3, 71))
    w = rng.integers(0, int(rng.integers(2, 5)), (ny, nx)).astype(np.int32) - 1
    w[rng.random((ny, nx)) < rng.uniform(0.0, 0.3)] = ND
    return w
