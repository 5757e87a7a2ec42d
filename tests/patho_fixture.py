"""tests/golden/patho_<case>.npz (tests/golden/make_golden_pathological.py) as the inputs and expected rasters of tests/downstream.py;
tests/golden/patholate_<case>.npz (make_golden_patholate.py) beside them for the five late tools (downstream.*_late)."""
import os

import numpy as np

import downstream as D

HERE = os.path.dirname(os.path.abspath(__file__))
DX = DY = 30.0
UPSTREAM = ("fel", "p", "sd8", "ang", "slp", "ad8", "ad8_nc", "sca", "sca_nc")


def names():
    return sorted(f[len("patho_"):-len(".npz")] for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("patho_") and f.endswith(".npz"))


def load(name):
    g = np.load(os.path.join(HERE, "golden", f"patho_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def inputs(g):
    """The downstream tools' inputs of the fixture: the reference's directions and the recorded extra inputs."""
    inp = {k: g[k] for k in ("fel", "p", "sd8", "ang", "slp")}
    inp["ad8"], inp["sca"] = g["ad8_nc"], g["sca_nc"]
    inp.update({k[3:]: g[k] for k in g if k.startswith("in_") and k not in ("in_outlets", "in_gauges")})
    inp["outlets"] = tuple(g["in_outlets"])
    inp["gauges"] = tuple(g["in_gauges"])
    return inp


def expected(g):
    """{key: raster} of the reference in the keys of downstream.reference (the -id text under gw_id)."""
    out = {k: g[k] for k in g if not k.startswith("in_") and k not in UPSTREAM and k not in ("dem", "index", "gw_id")}
    out["gw_id"] = str(g["gw_id"])
    return out


def restated(R, g):
    return D.reference(R, inputs(g), DX, DY, int(g["index"]))


def gpu(ctx, g):
    return D.single(ctx, inputs(g), DX, DY, int(g["index"]))


def late_names():
    return sorted(f[len("patholate_"):-len(".npz")] for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("patholate_") and f.endswith(".npz"))


def load_late(name):
    """(g, inp): the late fixture and the late tools' inputs - the reference's directions of patho_<name>.npz, the recorded inputs of both
    files, the avalanche's geometry (30 x 40 cells; the angles the reference's DinfFlowDir gave on them are recorded as in_ang_a)."""
    g = np.load(os.path.join(HERE, "golden", f"patholate_{name}.npz"), allow_pickle=False)
    g = {k: g[k] for k in g.files}
    inp = inputs(load(name))
    inp.update({k[3:]: g[k] for k in g if k.startswith("in_")})
    inp["aval_cells"] = D.PYTH
    inp["aval_geo"] = tuple(float(v) for v in g["geo"])
    inp["aval_direct"] = str(g["direct"])
    return g, inp


def expected_late(g, R, inp):
    """{key: raster} of the reference in the keys of downstream.reference_late; the taint masks beside them are the restatement's."""
    return dict({k: g[k] for k in g if not k.startswith("in_") and k not in ("index", "geo", "direct", "libc")}, **D.aval_taints(R, inp))
