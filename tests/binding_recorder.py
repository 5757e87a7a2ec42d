"""Drives every Context and StripPipeline stage method against a recording stub in place of the loaded library and returns what reached
the C boundary in a normal form: tests/test_binding_calls.py compares it with tests/golden/binding_calls.json, which
tests/golden/make_golden_binding_calls.py wrote from this same module.  No library is loaded and nothing touches a device: device rasters
are stand-in tensors, and torch.empty / torch.cuda.synchronize are replaced while a case runs.

Normal form of one call: the symbol, its arguments under the parameter names of include/taudem_amd.h, the number of torch.cuda.synchronize
calls and the shape of the return value.  A scalar is converted to the symbol's argtype first (so float(np.float32(x)) and the literal x
compare equal); a raster pointer becomes the name of the raster it addresses (`out<k>`: element k of the return value), NULL `null`, the
per-row cell sizes `rows[n]:<values>`, every other host array `<type>[n]:<values>`, the stats pointer `stats`."""
import contextlib
import ctypes as C
from unittest import mock

import numpy as np
import torch

from taudem_amd import _lib
from taudem_amd.api import Context
from taudem_amd.distributed import StripPipeline

NY, NX = 5, 7                 # Context rasters
NY_LOCAL = 4                  # strip arrays are (NY_LOCAL + 2, NX)
DEVICE = 0
CTX_HANDLE, COMM_HANDLE = 0x1000, 0x2000

# the parameter names of tdx_<tool>(...) in include/taudem_amd.h (the _dev form's are the same; _strip: see _names())
PARAMS = {
    "pitremove": "ctx dem nx ny dem_nodata mask fourway fel stats",
    "d8flowdir": "ctx fel nx ny fel_nodata dxc dyc p sd8 stats",
    "aread8": "ctx p nx ny p_nodata w w_nodata contcheck outlet_x outlet_y n_outlets ad8 stats",
    "gridnet": "ctx p nx ny p_nodata dxc dyc mask thresh outlet_x outlet_y n_outlets plen tlen gord stats",
    "threshold": "ctx ssa nx ny ssa_nodata mask thresh src stats",
    "d8flowpathextremeup": "ctx p nx ny p_nodata sa usemax contcheck outlet_x outlet_y n_outlets ssa stats",
    "dinfflowdir": "ctx fel nx ny fel_nodata dxc dyc ang slp stats",
    "areadinf": "ctx ang nx ny ang_nodata dxc dyc w contcheck outlet_x outlet_y n_outlets sca stats",
    "dinfdecayaccum": "ctx ang nx ny ang_nodata dxc dyc dm dm_nodata w contcheck outlet_x outlet_y n_outlets dsca stats",
    "dinfupdependence": "ctx ang nx ny ang_nodata dxc dyc dg dep stats",
    "dinfrevaccum": "ctx ang nx ny ang_nodata dxc dyc w w_nodata racc dmax stats",
    "dinfdistdown": "ctx ang nx ny ang_nodata dxc dyc fel fel_nodata src w w_nodata statmethod typemethod contcheck dd stats",
    "d8hdisttostrm": "ctx p nx ny p_nodata src src_nodata thresh dxc dyc dist stats",
    "gagewatershed": "ctx p nx ny p_nodata outlet_x outlet_y ids n_outlets gw placed iddown stats",
    "d8vdisttostrm": "ctx p nx ny p_nodata fel src src_nodata thresh dist stats",
    "flowdircond": "ctx p nx ny p_nodata z z_nodata zfdc stats",
    "slopeavedown": "ctx p nx ny p_nodata fel fel_nodata dxc dyc dn niter slpd stats",
    "dinfdistup": "ctx ang nx ny ang_nodata dxc dyc fel fel_nodata w w_nodata statmethod typemethod contcheck thresh du stats",
    "retlimflow": "ctx ang nx ny ang_nodata dxc dyc wg wg_nodata rc rc_nodata qrl stats",
    "dinfavalanche": "ctx ang nx ny ang_nodata dxc dyc fel fel_nodata ass ass_nodata thresh alpha path geo geographic rz dfs stats",
    "dinfconclimaccum": "ctx ang nx ny ang_nodata dxc dyc dm dm_nodata dg q q_nodata csol contcheck outlet_x outlet_y n_outlets ctpt stats",
    "dinftranslimaccum": "ctx ang nx ny ang_nodata dxc dyc tsup tsup_nodata tc tc_nodata cs cs_nodata contcheck outlet_x outlet_y n_outlets tla tdep ctpt stats",
    "catchhydrogeo": "ctx hand catch slp nx ny hand_nodata catch_nodata slp_nodata dxc dyc ids ncatch stages nheight count surface bed volume catcharea stats",
    "inundepth": "ctx hand catch mask nx ny hand_nodata catch_nodata mask_nodata dxc dyc ids depth nfc map area stats",
}
# host arrays the library reads or fills through a bare pointer: parameter -> (element type, the parameter(s) that hold its length, extra)
HOST_ARRAYS = {
    "outlet_x": (C.c_int32, ("n_outlets",), 0), "outlet_y": (C.c_int32, ("n_outlets",), 0), "ids": (C.c_int32, ("n_outlets", "ncatch", "nfc"), 0),
    "placed": (C.c_int32, ("n_outlets",), 1), "iddown": (C.c_int32, ("n_outlets",), 1),     # scratch of n_outlets + 1, zeroed
    "stages": (C.c_double, ("nheight",), 0), "depth": (C.c_float, ("nfc",), 0),
}
TYPE_TAGS = {C.c_int32: "i32", C.c_double: "f64", C.c_float: "f32"}


def _names(symbol):
    """The parameter names of a recorded symbol: the strip form takes the comm after the context, and the avalanche's row0 / ny_total."""
    tool = symbol[4:]
    strip = tool.endswith("_strip")
    names = PARAMS[tool.rsplit("_", 1)[0] if strip or tool.endswith("_dev") else tool].split()
    if strip:
        names.insert(1, "comm")
        if tool == "dinfavalanche_strip":
            names[names.index("rz"):names.index("rz")] = ["row0", "ny_total"]
    return names


class FakeDevice:
    type = "cuda"

    def __init__(self, index):
        self.index = index


class FakeTensor:
    """What the binding reads of a torch tensor, and an address of its own."""
    __module__ = "torch"          # the binding tells tensors from numpy arrays by the type's module

    def __init__(self, shape, dtype, cuda=True, contiguous=True, index=DEVICE):
        self.shape, self.dtype, self.is_cuda, self._contiguous, self.device = tuple(shape), dtype, cuda, contiguous, FakeDevice(index)
        self._mem = np.empty(8, np.uint8)

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return self._mem.ctypes.data


TORCH_DT = {np.float32: torch.float32, np.int16: torch.int16, np.int32: torch.int32}


def _address(a):
    return a.data_ptr() if isinstance(a, FakeTensor) else a.ctypes.data


class Recorder:
    """Stands in for the loaded library: every exported symbol returns 0 and records (symbol, arguments); host arrays are read at once."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        if symbol not in _lib.EXPORTED_SYMBOLS:
            raise AttributeError(symbol)

        def fn(*args):
            self.calls.append((symbol, self._snapshot(symbol, args)))
            return 0
        return fn

    @staticmethod
    def _snapshot(symbol, args):
        names, argtypes = _names(symbol), _lib._SIGNATURES[symbol][1]
        assert len(args) == len(names) == len(argtypes), f"{symbol}: {len(args)} arguments, the header has {len(names)}"
        raw, out = dict(zip(names, args)), {}
        rows = raw["ny"] + 2 if "comm" in raw else raw["ny"]

        def address(v):
            return v.value if isinstance(v, C.c_void_p) else v

        def array(v, ctype, n, tag):
            if address(v) is None:
                return "null"
            vals = (ctype * n).from_address(address(v))
            return f"{tag}[{n}]:" + ",".join(repr(x) for x in vals)

        for name, v, t in zip(names, args, argtypes):
            if name == "stats":
                out[name] = "stats" if type(v).__name__ == "CArgObject" else repr(v)
            elif t is not C.c_void_p:
                out[name] = t(v).value
            elif name in ("dxc", "dyc"):
                out[name] = array(v, C.c_double, rows, "rows")
            elif name == "geo":
                out[name] = array(v, C.c_double, 4, "f64")
            elif name in HOST_ARRAYS:
                ctype, lengths, extra = HOST_ARRAYS[name]
                n = int(next(raw[k] for k in lengths if k in raw))
                out[name] = array(v, ctype, n + extra, TYPE_TAGS[ctype]) if n >= 0 else ("null" if address(v) is None else "not null")
            else:
                out[name] = ("address", address(v))           # a raster, the context or the comm: named by resolve()
        return out


def resolve(args, known):
    """Replaces the addresses left in a snapshot - the ("address", value) entries - by their names in `known` (address -> name); gives [parameter, value] pairs in the
    order of the call."""
    return [[k, ("null" if v[1] is None else known.get(v[1], "unknown")) if isinstance(v, tuple) else v] for k, v in args.items()]


class Rasters:
    """The rasters of one case by name, numpy arrays (side "host") or stand-in tensors (side "device"), made on first use."""
    DTYPES = {"p": np.int16, "mask16": np.int16, "src16": np.int16, "ass": np.int16, "dg16": np.int16, "o_p": np.int16,
              "mask32": np.int32, "dg32": np.int32, "src32": np.int32, "catch": np.int32}

    def __init__(self, side, shape):
        self.side, self.shape, self.made = side, shape, {}

    def __call__(self, key, **fake):
        if key not in self.made:
            dt = self.DTYPES.get(key, np.float32)
            self.made[key] = FakeTensor(self.shape, TORCH_DT[dt], **fake) if self.side == "device" else np.zeros(self.shape, dt)
        return self.made[key]

    def known(self):
        return {_address(a): k for k, a in self.made.items()}


OUTLETS = (np.array([1, 5, 3], np.int32), np.array([2, 1, 4], np.int32))
GAUGES = OUTLETS + (np.array([7, 9, 8], np.int32),)
IDS = np.array([3, 1, 6, 40], np.int32)
STAGES = [0.0, 0.5, 2.0]
DEPTHS = np.array([1.5, 0.25, 4.0, -1.0], np.float32)
GEO = (1000.0, 5200.0, 30.0, 40.0)
DX = 30.0


def dy(rows):
    return 40.0 + 0.25 * np.arange(rows)


# tool -> f(c, r, o): o = every optional raster, outlets and out= given and every scalar set to a value of its own, with a scalar dx and a
# per-row dy; not o = none of them, the defaults, scalar dx and dy.  CONTEXT runs with stats=True.
CONTEXT = {
    "pitremove": lambda c, r, o: c.pitremove(r("dem"), -9998.0, r("mask16"), True, r("o_fel"), stats=True) if o else c.pitremove(r("dem"), stats=True),
    "d8flowdir": lambda c, r, o: (c.d8flowdir(r("fel"), -2.0e38, DX, dy(NY), True, (r("o_p"), r("o_sd8")), stats=True) if o
                                  else c.d8flowdir(r("fel"), dx=DX, dy=40.0, want_slope=False, stats=True)),
    "aread8": lambda c, r, o: (c.aread8(r("p"), -32767, r("w"), -9997.0, False, OUTLETS, r("o_ad8"), stats=True) if o else c.aread8(r("p"), stats=True)),
    "d8flowpathextremeup": lambda c, r, o: (c.d8flowpathextremeup(r("p"), r("sa"), -32767, False, False, OUTLETS, r("o_ssa"), stats=True) if o
                                            else c.d8flowpathextremeup(r("p"), r("sa"), stats=True)),
    "gridnet": lambda c, r, o: (c.gridnet(r("p"), -32767, DX, dy(NY), r("mask32"), 11, OUTLETS, stats=True) if o
                                else c.gridnet(r("p"), dx=DX, dy=40.0, stats=True)),
    "threshold": lambda c, r, o: c.threshold(r("ssa"), 12.5, -2.0, r("maskf"), stats=True) if o else c.threshold(r("ssa"), 3.0, stats=True),
    "dinfflowdir": lambda c, r, o: (c.dinfflowdir(r("fel"), -2.0e38, DX, dy(NY), (r("o_ang"), r("o_slp")), stats=True) if o
                                    else c.dinfflowdir(r("fel"), dx=DX, dy=40.0, stats=True)),
    "areadinf": lambda c, r, o: (c.areadinf(r("ang"), -2.5e38, DX, dy(NY), r("w"), False, OUTLETS, r("o_sca"), stats=True) if o
                                 else c.areadinf(r("ang"), dx=DX, dy=40.0, stats=True)),
    "dinfdecayaccum": lambda c, r, o: (c.dinfdecayaccum(r("ang"), r("dm"), -2.5e38, -9996.0, DX, dy(NY), r("w"), False, OUTLETS, r("o_dsca"), stats=True) if o
                                       else c.dinfdecayaccum(r("ang"), r("dm"), dx=DX, dy=40.0, stats=True)),
    "dinfupdependence": lambda c, r, o: (c.dinfupdependence(r("ang"), r("dg32"), -2.5e38, DX, dy(NY), stats=True) if o
                                         else c.dinfupdependence(r("ang"), r("dg32"), dx=DX, dy=40.0, stats=True)),
    "dinfrevaccum": lambda c, r, o: (c.dinfrevaccum(r("ang"), r("w"), -2.5e38, -9995.0, DX, dy(NY), stats=True) if o
                                     else c.dinfrevaccum(r("ang"), r("w"), dx=DX, dy=40.0, stats=True)),
    # with: the surface distance reads fel and the weights; without: the horizontal one reads neither, though fel is given
    "dinfdistdown": lambda c, r, o: (c.dinfdistdown(r("ang"), r("src16"), r("feld"), stat="max", kind="s", weights=r("w"), weights_nodata=-9994.0, contcheck=False,
                                                    dx=DX, dy=dy(NY), nodata=-2.5e38, fel_nodata=-2.0e38, stats=True) if o
                                     else c.dinfdistdown(r("ang"), r("src16"), r("feld"), kind="h", dx=DX, dy=40.0, stats=True)),
    "dinfdistup": lambda c, r, o: (c.dinfdistup(r("ang"), r("feld"), stat="min", kind="p", weights=r("w"), weights_nodata=-9994.0, contcheck=False, thresh=0.125,
                                                dx=DX, dy=dy(NY), nodata=-2.5e38, fel_nodata=-2.0e38, stats=True) if o
                                   else c.dinfdistup(r("ang"), dx=DX, dy=40.0, stats=True)),
    "retlimflow": lambda c, r, o: (c.retlimflow(r("ang"), r("wg"), r("rc"), dx=DX, dy=dy(NY), nodata=-2.5e38, wg_nodata=-9993.0, rc_nodata=-9992.0, stats=True) if o
                                   else c.retlimflow(r("ang"), r("wg"), r("rc"), dx=DX, dy=40.0, stats=True)),
    "dinfavalanche": lambda c, r, o: (c.dinfavalanche(r("ang"), r("feld"), r("ass"), thresh=0.25, alpha=17.0, direct=True, dx=DX, dy=dy(NY), geo=GEO, geographic=True,
                                                      nodata=-2.5e38, fel_nodata=-2.0e38, ass_nodata=-32766, stats=True) if o
                                      else c.dinfavalanche(r("ang"), r("feld"), r("ass"), dx=DX, dy=40.0, stats=True)),
    "d8hdisttostrm": lambda c, r, o: (c.d8hdisttostrm(r("p"), r("src32"), 13, dx=DX, dy=dy(NY), nodata=-32767, src_nodata=-2147483646, stats=True) if o
                                      else c.d8hdisttostrm(r("p"), r("src32"), dx=DX, dy=40.0, stats=True)),
    "d8vdisttostrm": lambda c, r, o: (c.d8vdisttostrm(r("p"), r("feld"), r("src32"), 13, nodata=-32767, src_nodata=-2147483646, stats=True) if o
                                      else c.d8vdisttostrm(r("p"), r("feld"), r("src32"), stats=True)),
    "gagewatershed": lambda c, r, o: c.gagewatershed(r("p"), GAUGES, nodata=-32767, stats=True) if o else c.gagewatershed(r("p"), OUTLETS, stats=True),
    "flowdircond": lambda c, r, o: c.flowdircond(r("p"), r("z"), nodata=-32767, z_nodata=-2.0e38, stats=True) if o else c.flowdircond(r("p"), r("z"), stats=True),
    "slopeavedown": lambda c, r, o: (c.slopeavedown(r("p"), r("feld"), 75.0, dx=DX, dy=dy(NY), niter=4, nodata=-32767, fel_nodata=-2.0e38, stats=True) if o
                                     else c.slopeavedown(r("p"), r("feld"), dx=DX, dy=40.0, stats=True)),
    "catchhydrogeo": lambda c, r, o: (c.catchhydrogeo(r("hand"), r("catch"), r("slp"), IDS, STAGES, dx=DX, dy=dy(NY), hand_nodata=-2.5e38, catch_nodata=-9991,
                                                      slp_nodata=-2.0, stats=True) if o
                                      else c.catchhydrogeo(r("hand"), r("catch"), r("slp"), IDS, STAGES, dx=DX, dy=40.0, stats=True)),
    "inundepth": lambda c, r, o: (c.inundepth(r("hand"), r("catch"), IDS, DEPTHS, mask=r("mask16"), area=True, dx=DX, dy=dy(NY), hand_nodata=-2.5e38, catch_nodata=-9991,
                                              mask_nodata=-32765, stats=True) if o
                                  else c.inundepth(r("hand"), r("catch"), IDS, DEPTHS, area=False, dx=DX, dy=40.0, stats=True)),
    "dinfconclimaccum": lambda c, r, o: (c.dinfconclimaccum(r("ang"), r("dm"), r("dg16"), r("q"), 2.5, -2.5e38, -9996.0, -9990.0, DX, dy(NY), False, OUTLETS, stats=True) if o
                                         else c.dinfconclimaccum(r("ang"), r("dm"), r("dg16"), r("q"), dx=DX, dy=40.0, stats=True)),
    "dinftranslimaccum": lambda c, r, o: (c.dinftranslimaccum(r("ang"), r("tsup"), r("tc"), r("cs"), -2.5e38, -9989.0, -9988.0, -9987.0, DX, dy(NY), False, OUTLETS,
                                                              stats=True) if o
                                          else c.dinftranslimaccum(r("ang"), r("tsup"), r("tc"), dx=DX, dy=40.0, stats=True)),
}
R = NY_LOCAL + 2
STRIP = {
    "pitremove": lambda s, r, o: s.pitremove(r("dem"), -9998.0, True, r("o_fel")) if o else s.pitremove(r("dem")),
    "d8flowdir": lambda s, r, o: s.d8flowdir(r("fel"), -2.0e38, DX, dy(R), (r("o_p"), r("o_sd8"))) if o else s.d8flowdir(r("fel"), dx=DX, dy=40.0),
    "aread8": lambda s, r, o: s.aread8(r("p"), -32767, r("w"), -9997.0, False, OUTLETS, r("o_ad8")) if o else s.aread8(r("p")),
    "d8flowpathextremeup": lambda s, r, o: s.d8flowpathextremeup(r("p"), r("sa"), -32767, False, False, OUTLETS) if o else s.d8flowpathextremeup(r("p"), r("sa")),
    "gridnet": lambda s, r, o: s.gridnet(r("p"), -32767, DX, dy(R), r("mask32"), 11, OUTLETS) if o else s.gridnet(r("p"), dx=DX, dy=40.0),
    "dinfflowdir": lambda s, r, o: s.dinfflowdir(r("fel"), -2.0e38, DX, dy(R), (r("o_ang"), r("o_slp"))) if o else s.dinfflowdir(r("fel"), dx=DX, dy=40.0),
    "areadinf": lambda s, r, o: s.areadinf(r("ang"), -2.5e38, DX, dy(R), r("w"), False, OUTLETS, r("o_sca")) if o else s.areadinf(r("ang"), dx=DX, dy=40.0),
    "dinfdecayaccum": lambda s, r, o: (s.dinfdecayaccum(r("ang"), r("dm"), -2.5e38, -9996.0, DX, dy(R), r("w"), False, OUTLETS, r("o_dsca")) if o
                                       else s.dinfdecayaccum(r("ang"), r("dm"), dx=DX, dy=40.0)),
    "dinfupdependence": lambda s, r, o: s.dinfupdependence(r("ang"), r("dg32"), -2.5e38, DX, dy(R)) if o else s.dinfupdependence(r("ang"), r("dg32"), dx=DX, dy=40.0),
    "dinfrevaccum": lambda s, r, o: s.dinfrevaccum(r("ang"), r("w"), -2.5e38, -9995.0, DX, dy(R)) if o else s.dinfrevaccum(r("ang"), r("w"), dx=DX, dy=40.0),
    "dinfdistdown": lambda s, r, o: (s.dinfdistdown(r("ang"), r("src16"), r("feld"), stat="max", kind="s", weights=r("w"), weights_nodata=-9994.0, contcheck=False,
                                                    dx=DX, dy=dy(R), nodata=-2.5e38, fel_nodata=-2.0e38) if o
                                     else s.dinfdistdown(r("ang"), r("src16"), r("feld"), kind="h", dx=DX, dy=40.0)),
    "dinfdistup": lambda s, r, o: (s.dinfdistup(r("ang"), r("feld"), stat="min", kind="p", weights=r("w"), weights_nodata=-9994.0, contcheck=False, thresh=0.125,
                                                dx=DX, dy=dy(R), nodata=-2.5e38, fel_nodata=-2.0e38) if o
                                   else s.dinfdistup(r("ang"), dx=DX, dy=40.0)),
    "retlimflow": lambda s, r, o: (s.retlimflow(r("ang"), r("wg"), r("rc"), dx=DX, dy=dy(R), nodata=-2.5e38, wg_nodata=-9993.0, rc_nodata=-9992.0) if o
                                   else s.retlimflow(r("ang"), r("wg"), r("rc"), dx=DX, dy=40.0)),
    "dinfavalanche": lambda s, r, o: (s.dinfavalanche(r("ang"), r("feld"), r("ass"), row0=8, ny_total=21, thresh=0.25, alpha=17.0, direct=True, dx=DX, dy=dy(R), geo=GEO,
                                                      geographic=True, nodata=-2.5e38, fel_nodata=-2.0e38, ass_nodata=-32766) if o
                                      else s.dinfavalanche(r("ang"), r("feld"), r("ass"), row0=0, ny_total=NY_LOCAL, dx=DX, dy=40.0)),
    "d8hdisttostrm": lambda s, r, o: (s.d8hdisttostrm(r("p"), r("src32"), 13, dx=DX, dy=dy(R), nodata=-32767, src_nodata=-2147483646) if o
                                      else s.d8hdisttostrm(r("p"), r("src32"), dx=DX, dy=40.0)),
    "d8vdisttostrm": lambda s, r, o: (s.d8vdisttostrm(r("p"), r("feld"), r("src32"), 13, nodata=-32767, src_nodata=-2147483646) if o
                                      else s.d8vdisttostrm(r("p"), r("feld"), r("src32"))),
    "gagewatershed": lambda s, r, o: s.gagewatershed(r("p"), GAUGES, nodata=-32767) if o else s.gagewatershed(r("p"), GAUGES),
    "flowdircond": lambda s, r, o: s.flowdircond(r("p"), r("z"), nodata=-32767, z_nodata=-2.0e38) if o else s.flowdircond(r("p"), r("z")),
    "slopeavedown": lambda s, r, o: (s.slopeavedown(r("p"), r("feld"), 75.0, 4, dx=DX, dy=dy(R), nodata=-32767, fel_nodata=-2.0e38) if o
                                     else s.slopeavedown(r("p"), r("feld"), 50.0, 2, dx=DX, dy=40.0)),
    "dinfconclimaccum": lambda s, r, o: (s.dinfconclimaccum(r("ang"), r("dm"), r("dg16"), r("q"), 2.5, -2.5e38, -9996.0, -9990.0, DX, dy(R), False, OUTLETS) if o
                                         else s.dinfconclimaccum(r("ang"), r("dm"), r("dg16"), r("q"), dx=DX, dy=40.0)),
    "dinftranslimaccum": lambda s, r, o: (s.dinftranslimaccum(r("ang"), r("tsup"), r("tc"), r("cs"), -2.5e38, -9989.0, -9988.0, -9987.0, DX, dy(R), False, OUTLETS) if o
                                          else s.dinftranslimaccum(r("ang"), r("tsup"), r("tc"), dx=DX, dy=40.0)),
}
KINDS = {"context": CONTEXT, "context_dev": CONTEXT, "strip": STRIP}
CASES = [(kind, tool, o) for kind, table in KINDS.items() for tool in table for o in (True, False)]


def case_id(kind, tool, o):
    return f"{kind}/{tool}-{'with' if o else 'without'}"


class FakeComm:
    def ptr(self):
        return C.c_void_p(COMM_HANDLE)


def make_context(recorder):
    """A Context over the recorder: no library, no device."""
    ctx = Context.__new__(Context)
    ctx._lib, ctx._h, ctx._owned, ctx.device = recorder, C.c_void_p(CTX_HANDLE), False, DEVICE
    return ctx


@contextlib.contextmanager
def no_device():
    """torch.empty gives stand-in tensors and torch.cuda.synchronize counts its calls (the yielded list holds one entry per call)."""
    syncs = []

    def empty(shape, dtype=None, device=None):
        return FakeTensor(shape, dtype)

    with mock.patch.object(torch, "empty", empty), mock.patch.object(torch.cuda, "synchronize", lambda device=None: syncs.append(device)):
        yield syncs


def subject(kind, recorder):
    """(the object whose stage methods a case calls, its rasters)."""
    ctx = make_context(recorder)
    if kind == "strip":
        return StripPipeline(ctx, FakeComm(), NX, NY_LOCAL), Rasters("device", (NY_LOCAL + 2, NX))
    return ctx, Rasters("host" if kind == "context" else "device", (NY, NX))


def _describe(x):
    if isinstance(x, dict):
        return "stats"
    if x is None:
        return "none"
    return f"{str(x.dtype).replace('torch.', '')}{list(x.shape)}"


def run_case(kind, tool, o):
    """The normal form of what one case sent to the library."""
    rec = Recorder()
    with no_device() as syncs:
        sub, rasters = subject(kind, rec)
        ret = KINDS[kind][tool](sub, rasters, o)
    ret = ret if isinstance(ret, tuple) else (ret,)
    assert len(rec.calls) == 1, f"{len(rec.calls)} library calls"
    symbol, args = rec.calls[0]
    known = {CTX_HANDLE: "ctx", COMM_HANDLE: "comm"}
    known.update({_address(x): f"out{k}" for k, x in enumerate(ret) if isinstance(x, FakeTensor) or (isinstance(x, np.ndarray) and x.size > 0)})
    known.update(rasters.known())
    return {"symbol": symbol, "args": resolve(args, known), "syncs": len(syncs), "returns": [_describe(x) for x in ret]}


def _type_name(t):
    """A ctypes type by what it is rather than by the platform's spelling: c_long and c_longlong are both int64 where they have 8 bytes."""
    if t is None:
        return "None"
    if hasattr(t, "_type_") and isinstance(t._type_, str) and t._type_ in "bhilq":
        return f"int{8 * C.sizeof(t)}"
    if hasattr(t, "_type_") and isinstance(t._type_, str) and t._type_ in "BHILQ":
        return f"uint{8 * C.sizeof(t)}"
    return t.__name__


def signatures():
    """restype and argtypes of every exported symbol."""
    return {s: [_type_name(_lib._SIGNATURES[s][0]), [_type_name(t) for t in _lib._SIGNATURES[s][1]]] for s in sorted(_lib.EXPORTED_SYMBOLS)}


def record_all():
    return {"calls": {case_id(*c): run_case(*c) for c in CASES}, "signatures": signatures()}
