"""The Python binding, pinned at the C boundary without a library or a GPU (tests/binding_recorder.py): every Context stage method (numpy
rasters: the host form; stand-in tensors: the device form) and every StripPipeline stage method sends the symbol, the arguments in the
header's order, and makes the number of torch.cuda.synchronize calls that tests/golden/binding_calls.json records - written by
tests/golden/make_golden_binding_calls.py before the bindings were folded onto one call frame.  Rasters are 5 x 7 and strips 4 owned rows of
7 (arrays of 6 x 7): not square, and the smallest where halo and owned rows differ.  Each tool runs with every optional raster, the outlets
and out= given and every scalar set to a value of its own (scalar dx, per-row dy), and with none of them and the defaults (scalar dx, dy).
_lib._SIGNATURES is held to the recorded restype / argtypes of every exported symbol.

A raster of the wrong dtype, not contiguous, of the wrong shape or on the other side from the first input is refused with ValueError before
any library call.  test_other_side_output_is_rejected and test_strip_outlets_are_checked are the cases the call frame newly rejects: they
are the only tests here that fail on the commit the golden file was recorded at."""
import json
import os

import numpy as np
import pytest
import torch

import binding_recorder as B
from conftest import GOLDEN_DIR

with open(os.path.join(GOLDEN_DIR, "binding_calls.json")) as f:
    GOLDEN = json.load(f)


@pytest.mark.parametrize("kind,tool,o", B.CASES, ids=[B.case_id(*c) for c in B.CASES])
def test_call_reaches_the_library_as_recorded(kind, tool, o):
    got, want = B.run_case(kind, tool, o), GOLDEN["calls"][B.case_id(kind, tool, o)]
    assert got["symbol"] == want["symbol"]
    assert got["args"] == want["args"]
    assert got["syncs"] == want["syncs"] and got["returns"] == want["returns"]


def test_every_stage_method_is_driven():
    from taudem_amd.api import Context
    from taudem_amd.distributed import StripPipeline

    stages = lambda cls, skip: {n for n, v in vars(cls).items() if callable(v) and not n.startswith("_")} - skip  # noqa: E731
    assert stages(Context, {"borrow", "close", "release_scratch", "set_option", "segments", "synth_dem"}) == set(B.CONTEXT) and len(B.CONTEXT) == 24
    assert stages(StripPipeline, {"empty", "local_outlets"}) == set(B.STRIP)
    assert set(GOLDEN["calls"]) == {B.case_id(*c) for c in B.CASES}
    symbols = {c["symbol"] for c in GOLDEN["calls"].values()}
    assert symbols == {f"tdx_{t}{s}" for t in B.CONTEXT for s in ("", "_dev")} | {f"tdx_{t}_strip" for t in B.STRIP}


def test_signatures_are_the_recorded_ones():
    assert B.signatures() == GOLDEN["signatures"]


class _DefaultStats:
    """A Context whose stage methods are called without the stats argument."""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return lambda *a, stats=None, **k: getattr(self._ctx, name)(*a, **k)


@pytest.mark.parametrize("tool", list(B.CONTEXT))
def test_stats_flag_only_adds_the_stats(tool):
    """Without stats (the default) a Context method returns what stats=True does less the trailing dict, a single output bare."""
    with B.no_device():
        ctx, r = B.subject("context", B.Recorder())
        full, bare = B.CONTEXT[tool](ctx, r, False), B.CONTEXT[tool](_DefaultStats(ctx), r, False)
    assert isinstance(full, tuple) and isinstance(full[-1], dict) and "ms_total" in full[-1]
    bare = bare if len(full) > 2 else (bare,)
    assert isinstance(bare, tuple) and [B._describe(x) for x in bare] == [B._describe(x) for x in full[:-1]]


def _fails_before_any_call(kind, call):
    rec = B.Recorder()
    with B.no_device():
        sub, r = B.subject(kind, rec)
        with pytest.raises(ValueError):
            call(sub, r)
    assert rec.calls == []


def _bad(kind, r, key, what):
    """Raster `key` of the case with one thing wrong with it."""
    dev, (ny, nx) = kind != "context", r.shape
    if what == "dtype":
        return B.FakeTensor(r.shape, torch.float64) if dev else np.zeros(r.shape, np.float64)
    if what == "contiguity":
        return B.FakeTensor(r.shape, torch.float32, contiguous=False) if dev else np.zeros((ny, 2 * nx), np.float32)[:, ::2]
    if what == "shape":
        return B.FakeTensor((nx, ny), torch.float32) if dev else np.zeros((nx, ny), np.float32)
    assert what == "side"
    if kind == "context":
        return B.FakeTensor(r.shape, torch.float32)
    return np.zeros(r.shape, np.float32) if kind == "context_dev" else B.FakeTensor(r.shape, torch.float32, cuda=False)


@pytest.mark.parametrize("what", ["dtype", "contiguity", "shape", "side"])
@pytest.mark.parametrize("kind", list(B.KINDS))
def test_bad_raster_is_rejected(kind, what):
    """A required second input (sa of d8flowpathextremeup) and an optional one (weights of aread8)."""
    _fails_before_any_call(kind, lambda s, r: s.d8flowpathextremeup(r("p"), _bad(kind, r, "sa", what)))
    _fails_before_any_call(kind, lambda s, r: s.aread8(r("p"), weights=_bad(kind, r, "w", what)))


@pytest.mark.parametrize("what", ["dtype", "contiguity"])
@pytest.mark.parametrize("kind", list(B.KINDS))
def test_bad_first_raster_is_rejected(kind, what):
    _fails_before_any_call(kind, lambda s, r: s.dinfflowdir(_bad(kind, r, "fel", what)))


def test_strip_rejects_host_and_misshapen_first_raster():
    _fails_before_any_call("strip", lambda s, r: s.dinfflowdir(B.FakeTensor((B.NY_LOCAL, B.NX), torch.float32)))
    _fails_before_any_call("strip", lambda s, r: s.dinfflowdir(B.FakeTensor(r.shape, torch.float32, cuda=False)))


@pytest.mark.parametrize("tool,second", [("d8flowdir", "o_sd8"), ("dinfflowdir", "o_slp")])
@pytest.mark.parametrize("kind", ["context", "context_dev"])
def test_other_side_output_is_rejected(kind, tool, second):
    """out=(first, second) with the second output on the other side from fel: before the call frame its side was not looked at, and a
    device fel with a host second output handed a host pointer to the _dev entry point."""
    other = B.Rasters("device" if kind == "context" else "host", (B.NY, B.NX))
    _fails_before_any_call(kind, lambda s, r: getattr(s, tool)(r("fel"), out=(r("o_p" if tool == "d8flowdir" else "o_ang"), other(second))))


def test_strip_outlets_are_checked():
    """Strip outlets get Context's check: two 1-D index arrays of one length."""
    _fails_before_any_call("strip", lambda s, r: s.aread8(r("p"), outlets=([1, 2], [1])))
    _fails_before_any_call("context", lambda s, r: s.aread8(r("p"), outlets=([1, 2], [1])))
    _fails_before_any_call("strip", lambda s, r: s.gagewatershed(r("p"), ([1, 2], [1, 2], [1])))
