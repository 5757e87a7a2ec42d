"""Every compute entry point of the C ABI - each tool in its host, _dev and _strip form - rejects a null context with TDX_ERR_ARG
and its own "<symbol>: bad argument" text before it touches HIP.  No GPU is needed: the library loads without one (tests/test_host.py)
and the context test comes first in every entry point."""
import os
import re

import pytest

import taudem_amd as T
from taudem_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry points whose text for a null context is not "<symbol>: bad argument" (none today; the table keeps whatever the library said
# when this test was written, it is not a list of things to fix)
OTHER_TEXT = {}


def _compute_symbols():
    """A tool is a name the header declares both as tdx_x and as tdx_x_dev; its compute calls are those two and tdx_x_strip where declared."""
    text = open(os.path.join(ROOT, "include", "taudem_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = set(re.findall(r"\b(tdx_[a-z0-9_]+)\s*\(", text))
    tools = sorted(s for s in syms if s + "_dev" in syms)
    return [t + form for t in tools for form in ("", "_dev", "_strip") if t + form in syms]


SYMBOLS = _compute_symbols()


def test_compute_symbol_list():
    assert len(SYMBOLS) == 71 and len([s for s in SYMBOLS if s.endswith("_dev")]) == 24   # 24 tools; tdx_threshold has no strip form
    assert set(SYMBOLS) <= set(_lib.EXPORTED_SYMBOLS)
    assert not set(OTHER_TEXT) - set(SYMBOLS)


@pytest.mark.parametrize("sym", SYMBOLS)
def test_null_context_is_a_bad_argument(sym):
    fn = getattr(T.load(), sym)
    rc = fn(*[t() for t in fn.argtypes])   # null context, null pointers, zeros
    assert rc == _lib.TDX_ERR_ARG
    assert _lib.last_error(None) == OTHER_TEXT.get(sym, sym + ": bad argument")
