"""The restatement of the five terrain-index tools (tests/indices/indices_restate.c) against what the real tools wrote (tests/golden/indices_*.npz, made by
tests/golden/make_golden_indices.py), by the three rules of tests/indices_model.py: SlopeAreaRatio, SetRegion, LengthArea and every nodata / not-written
pattern exact; TWI within 1 float ulp and SlopeArea within 6 of the correctly rounded value the restatement gives, with at most 1 % of a run's cells
different at all.  The measured figures are printed before anything is asserted.  The margins the fixtures were chosen for are held too.  No GPU is needed."""
import numpy as np
import pytest

import indices_model as M


@pytest.fixture(scope="module")
def restate(tmp_path_factory):
    return M.compile(tmp_path_factory.mktemp("indices_restate"))


@pytest.mark.parametrize("name", M.FIXTURES)
def test_restatement_against_the_reference(restate, name):
    gold, stats, glibc = M.load_golden(name)
    runs = M.all_runs(name)
    assert sorted(gold) == sorted(k for k, _, _ in runs)
    for key, tool, r in runs:
        got, want = gold[key], restate.run(tool, r)
        assert got.dtype == want.dtype and got.shape == want.shape, (name, key)
        if tool in ("sar", "setregion", "la"):
            assert M.same_bits(got, want), f"{name} {key}: {int(np.sum(got != want))} cells differ from the real tool"
            continue
        d = M.ulp_distance(got, want)
        share = float((d != 0).mean())
        print(f"indices {name} {key}: real tool ({glibc}) against the correctly rounded value: max {int(d.max())} ulp, {100 * share:.4f} % of the cells differ "
              f"(stored: {stats[key]['max_ulp']:.0f} ulp, {100 * stats[key]['diff_share']:.4f} %)")
        assert np.array_equal(got == -1.0, want == -1.0) and np.array_equal(np.isnan(got), np.isnan(want)), (name, key, "nodata or NaN pattern")
        assert d.max() <= (M.TWI_ULP if tool == "twi" else M.SA_ULP), (name, key)
        assert share <= M.DIFF_SHARE_CAP and stats[key]["diff_share"] <= M.DIFF_SHARE_CAP, (name, key)
        assert d.max() == stats[key]["max_ulp"] and share == stats[key]["diff_share"], (name, key, "the stored statistics are not this host's restatement's")


@pytest.mark.parametrize("name", M.FIXTURES)
def test_no_committed_cell_on_a_knife_edge(restate, name):
    for key, tool, r in M.all_runs(name) + ([M.fractional_run()] if name == "plain" else []):
        if tool == "twi":
            margin = restate.twi(r["slp"], r["sca"])[1]
        elif tool == "sa":
            margin = restate.sa(r["slp"], r["sca"], *r["par"])[1]
        elif tool == "la":
            ss, margin, fac, thr, ad8i = restate.lengtharea(r["plen"], r["ad8"], *r["par"])
            margin = margin[ss != M.SS_NOT_WRITTEN]
            if not (r["par"][1] == 1.0 or r.get("planted")):
                d = M.ulp_distance(ad8i.astype(np.float32), thr)
                near = (ss != M.SS_NOT_WRITTEN) & np.isfinite(thr) & (d <= 2) & (r["plen"] != 0) & (r["plen"] != 1)
                assert not near.any(), (name, key, "float(ad8) within 2 ulp of a threshold a libm could move")
        else:
            continue
        assert margin.size == 0 or margin.min() >= M.MARGIN_MIN, (name, key, float(margin.min()))


def test_planted_thresholds_hold_greater_or_equal():
    gold = M.load_golden("hand")[0]
    runs = {k: r for k, _, r in M.hand_runs()}
    r, g = runs["planted_la_half_one"], gold["planted_la_half_one"]
    on = r["ad8"] == np.float32(0.5) * r["plen"]
    assert on.sum() >= 6 and np.all(g[on & (r["plen"] >= 0)] == 1)                      # ad8 == M * plen: >= holds, > would not
    assert g[0, 6] == 0 and g[0, 7] == 1 and g[1, 0] == -32768 and g[1, 1] == -32768    # below, above, a negative and a NaN length: not written
    g2 = gold["planted_la_two"]
    assert g2.tolist() == [[1, 1, 0, 1, 0, 1]]


def test_what_the_hand_built_rasters_pin():
    gold = M.load_golden("hand")[0]
    slp, sca = M.special_terrain()
    twi, sar, sa = gold["special_twi"], gold["special_sar"], gold["special_sa_negexp"]
    assert twi[0, :7].tolist() == [-1.0] * 7 and twi[0, 7] == -np.inf            # zeros, nodata on either side, NaN: nodata; inf slope: ln 0
    assert twi[2, 1] == np.inf and abs(twi[2, 2] - np.log(1e-40)) < 1e-3         # a quotient that overflows, a subnormal one
    assert twi[2, 3] == -1.0 and twi[2, 4] == -1.0                               # sca within MINEPS of nodata; just outside it but negative
    assert sar[2, 3] == -1.0 and sar[2, 4] == np.float32(0.5) / np.float32(-0.99998)   # ... which SlopeAreaRatio divides by
    assert sar[0, 3] == np.float32(-1.0) / np.float32(30.0)                      # a nodata slope flows through
    assert np.isnan(sar[0, 2]) and sar[0, 1] == np.inf and np.signbit(sar[1, 5]) and sar[1, 5] == 0 and sar[1, 6] == -np.inf
    assert sa[0, 3] == -1.0 and sa[0, 4] == -1.0 and sa[0, 5] == -1.0            # negative values and NaN fail the >= 0 test
    assert sa[0, 1] == np.inf and np.isnan(sa[0, 2])                             # pow(0, -0.75) = inf; 0 * inf
    z = gold["special_sa_zeroexp"]
    assert z[0, 0] == np.float32(30.0) ** np.float32(1.5) or abs(z[0, 0] - 30.0 ** 1.5) < 1e-4   # pow(0, 0) = 1
    assert np.isnan(gold["special_sa_default"][2, 0]) or gold["special_sa_default"][2, 0] == np.inf  # inf^2 * inf


def test_setregion_hand_rasters():
    gold = M.load_golden("hand")[0]
    g = gold["hole_blocks"]
    centres = g[2, 2::5]
    assert centres[:8].tolist() == [1] * 8 and centres[8:].tolist() == [int(M.MISSINGLONG)] * 4
    assert (g == 1).sum() == 8 + 12 + 1   # the eight centres, the twelve live cells (data in p or in gw) and the hole block 8's neighbour flows away INTO
    assert g[2, 44] == 1
    e = gold["edge_holes"]
    assert np.all(e[1:5, 1:6] == 5) and (e[0] == 5).any() and (e[-1] == 5).any() and e[0, 0] == int(M.MISSINGLONG) and e[5, 0] == 5
