"""tests/netlayer_model.py - the stream network layer and CatchOutlets restated in Python - against the records of the real tools
(tests/golden/netlayer_*.npz).  net_rows on the rows of the committed -tree / -coord text gives the recorded layer bit for bit wherever the generator
found that the text keeps every float of the links (exact_<v>: four of the five cases and all hand-built rasters); with the recorded vertices in place of
the text's six decimals it does on every case, the geographic one included, whose lengths go through the restated tiffIO::geotoLength.  catch_outlets on
the recorded layer gives every CatchOutlets record, feature for feature.  No GPU is needed."""
import numpy as np
import pytest

import netlayer_model as N
import streamnet_model as M

SMALL = [str(n) for n in N.load("small")["names"]]
RUNS = [(name, "") for name in M.CASES] + [("small", n + "_") for n in SMALL]


def _inputs(name, prefix):
    """(the records, the streamnet fixture, p, geotransform, geographic) of a case or of a hand-built raster"""
    rec, fix = N.load(name), M.load_golden(name)
    if name == "small":
        return rec, fix, M.small_rasters()[prefix[:-1]][0], M.SMALL_GT, False
    return rec, fix, fix["p"], tuple(fix["gt"]), name == "geographic"


@pytest.mark.parametrize("name,prefix", RUNS)
def test_net_rows_equal_the_record(name, prefix):
    rec, fix, _, _, geographic = _inputs(name, prefix)
    for v in N.VARIANTS:
        want = N.parse_lines(N.text(rec[f"{prefix}net_{v}"]))
        tree, coord = N.rows_of_text(fix[f"{prefix}tree_{v}"], fix[f"{prefix}coord_{v}"])
        assert len(want[1]) == len(tree)
        if not len(tree):
            continue
        assert bool(rec[f"{prefix}exact_{v}"]) == N.same_layer(N.net_rows(tree, coord, geographic), want), (name, prefix, v)
        assert bool(rec[f"{prefix}exact_{v}"]) or geographic   # only degrees lose something in six decimals
        for t, ln in zip(tree, want[1]):   # the vertices the tool handed over, which the record holds with 17 digits
            assert np.allclose(coord[t[1]:t[2] + 1, :2], ln[::-1], rtol=0, atol=1e-6)
            coord[t[1]:t[2] + 1, :2] = ln[::-1]
        assert N.same_layer(N.net_rows(tree, coord, geographic), want), (name, prefix, v)


@pytest.mark.parametrize("name,prefix", RUNS)
def test_catch_outlets_equal_the_records(name, prefix):
    rec, _, p, gt, _ = _inputs(name, prefix)
    n = 0
    for v in N.VARIANTS:
        if f"{prefix}co_params_{v}" not in rec:
            continue
        fields, lines = N.parse_lines(N.text(rec[f"{prefix}net_{v}"]))
        for k, (md, ma, gw) in enumerate(rec[f"{prefix}co_params_{v}"]):
            if f"{prefix}co_{v}_{k}" in rec:
                assert N.catch_outlets(fields, lines, p, gt, md, ma, int(gw)) == N.parse_points(N.text(rec[f"{prefix}co_{v}_{k}"])), (name, prefix, v, k)
                n += 1
        if v == "plain" and f"{prefix}co_plain_pzero" in rec:
            cx, cy = rec[f"{prefix}pzero_cell"]
            pz = p.copy()
            pz[cy, cx] = 0
            seen = {}
            got = N.catch_outlets(fields, lines, pz, gt, 0.0, 0.0, 1, seen)
            assert got == N.parse_points(N.text(rec[f"{prefix}co_plain_pzero"])) and seen["bad_p"] >= 1
            assert len(got) < len(N.parse_points(N.text(rec[f"{prefix}co_plain_0"])))   # that outlet link and all above it are not written
            n += 1
    assert n >= (9 if name != "small" else 0)


def test_the_records_hold_what_they_are_there_for():
    seen, ids = {}, set()
    for name, prefix in RUNS:
        rec, _, p, gt, _ = _inputs(name, prefix)
        for v in N.VARIANTS:
            if f"{prefix}co_params_{v}" not in rec:
                continue
            fields, lines = N.parse_lines(N.text(rec[f"{prefix}net_{v}"]))
            for k, (md, ma, gw) in enumerate(rec[f"{prefix}co_params_{v}"]):
                if f"{prefix}co_{v}_{k}" in rec:
                    out = N.catch_outlets(fields, lines, p, gt, md, ma, int(gw), seen)
                    ids |= {o[2]["Id"] for o in out[:1]}
    assert seen["mindist"] and seen["minarea"] and seen["stays"] and ids - {1}
