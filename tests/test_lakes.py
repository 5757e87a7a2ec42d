"""The lake generator (tests/lakes.py) does what it claims: from the queue and masks of the first flat iteration (the model of
flatk::classify_stream_kernel) and the blocks as flatk::find_blocks_kernel defines them, every lake holds the blocks it was built for, and the first
ring cells to hold a level are the ones asked for - so that tests/test_gpu_open_water.py cannot quietly degrade to "no blocks"."""
import pytest

import lakes as LK

WAVE0 = set(range(0, 64)) | set(range(256, 320)) | set(range(512, 576))   # ring positions tid + 256 u of wave 0 in LevelOpT::macro_update


def near(E, j, lake, ring1):
    """every level-1 ring cell is within one cell (chessboard) of ring cell (E, j), which holds level 1 itself"""
    y, x = lake.ring_cell(E, j)
    cells = {lake.ring_cell(e, i) for e in range(4) for i in ring1[e]}
    assert (y, x) in cells, (E, j, ring1)
    far = [c for c in cells if max(abs(c[0] - y), abs(c[1] - x)) > 1]
    assert not far, (E, j, far[:4])


def check(z, lake, whole=False):
    m = LK.lake_model(z, lake, whole=whole)
    want = {(tx, ty): k for tx, ty, k in lake.blocks}
    for field in ("fall", "rise"):
        assert m[field]["blocks"] == want, (field, lake, m[field]["blocks"])
    if lake.margin == 0:
        for (E, j) in lake.fall[:1] if len(lake.fall) == 1 else ():
            near(E, j, lake, m["fall"]["ring1"])
    for (E, j) in lake.rise[:1]:
        near(E, j, lake, m["rise"]["ring1"])
        for e in range(4):   # the rock is incrise's only way in: every other ring cell is at least three cells from the wall
            assert set(m["rise"]["ring1"][e]) <= {i for i in range(lake.ring_len(e)) if max(abs(a - b) for a, b in zip(lake.ring_cell(e, i), lake.ring_cell(E, j))) <= 1}
    if not lake.fall and not lake.nodata:
        assert m["fall"]["seeds"] == 0 and m["fall"]["queued"] > 0, "an undrained lake has no incfall seed"
    return m


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("source", ["fall", "rise"])
def test_sweep_lakes_hold_their_blocks_and_first_levels(k, source):
    regions_x = 6 if k == 8 else 8
    lakes = LK.sweep_lakes(k, source, regions_x)
    assert len(lakes) == 4 * len(LK.positions(k))
    z, lakes2 = LK.sweep_raster(k, source)
    assert [(l.tx, l.ty) for l in lakes2] == [(l.tx, l.ty) for l in lakes]
    for lake in lakes2:
        check(z, lake)


def test_race_lakes_are_one_sided():
    z, lakes = LK.race_raster()
    for lake in lakes:
        m = check(z, lake)
        (E, j), (E2, j2) = lake.fall
        ring1 = m["fall"]["ring1"]
        assert ring1[E] and not (set(ring1[E]) & WAVE0), (lake, ring1[E])    # edge E's seeds: none in wave 0's positions
        assert min(ring1[E]) >= 64
        assert set(ring1[E2]) == {j2 - 1, j2, j2 + 1}, lake                   # the other edge holds a level from the start


@pytest.mark.parametrize("name", sorted(LK.SHAPES))
def test_shape_lakes_hold_their_blocks(name):
    z, lakes = LK.shapes_raster(name)
    ny, nx = z.shape
    c = LK.classify(z)
    for field, mask in (("fall", c["fm"]), ("rise", c["rm"])):
        blocks, _ = LK.find_blocks(LK.full_tiles(mask))
        want = {(tx, ty): k for lake in lakes for tx, ty, k in lake.blocks}
        assert blocks == want, (name, field, blocks, want)
        # a partial last tile row / column is never part of a block
        assert all((tx + k) * 64 <= nx and (ty + k) * 64 <= ny for (tx, ty), k in blocks.items())
    assert ((-(-nx // 64)) % 8 == 0) == name.startswith("vec")   # tiles_x as the tile engine counts them
    for lake in lakes:
        check(z, lake, whole=True)
    assert c["q"].sum() > z.size // 16   # a dense first queue: DinfFlowDir's streaming classification
