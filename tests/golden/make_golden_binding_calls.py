"""Records what every Context and StripPipeline stage method sends to the library - symbol, arguments in the header's order, number of
synchronisations, shape of the return value - and the restype / argtypes of every exported symbol, into binding_calls.json:

    python tests/golden/make_golden_binding_calls.py

Needs neither the built library nor a GPU: tests/binding_recorder.py puts a recording stub in the library's place.  The file was written
at the commit before the bindings were folded onto one call frame; tests/test_binding_calls.py holds the bindings to it.  A second run
writes the same bytes.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import binding_recorder as B  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "binding_calls.json")


def dump(rec):
    """The record as JSON with one call argument and one signature per line, keys sorted."""
    j = json.dumps
    calls = []
    for cid in sorted(rec["calls"]):
        c = rec["calls"][cid]
        args = ",\n".join(f"    {j(a)}" for a in c["args"])
        calls.append(f'  {j(cid)}: {{"symbol": {j(c["symbol"])}, "syncs": {j(c["syncs"])}, "returns": {j(c["returns"])}, "args": [\n{args}\n  ]}}')
    sigs = ",\n".join(f"  {j(s)}: {j(v)}" for s, v in sorted(rec["signatures"].items()))
    return '{\n "calls": {\n' + ",\n".join(calls) + '\n },\n "signatures": {\n' + sigs + "\n }\n}\n"


if __name__ == "__main__":
    rec = B.record_all()
    with open(OUT, "w") as f:
        f.write(dump(rec))
    assert json.load(open(OUT)) == rec
    print(f"{len(rec['calls'])} calls, {len(rec['signatures'])} signatures, {os.path.getsize(OUT)} bytes")
