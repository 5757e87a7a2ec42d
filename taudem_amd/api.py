"""In-memory interface to the HIP hot path (one :class:`Context` per GPU / process rank).

Every method accepts either numpy arrays (host buffers: the library stages them over PCIe) or torch
CUDA tensors on the context's device (HBM-resident: no copies, the benchmark path).  Array layout,
dtypes and nodata conventions are the reference's (include/taudem_amd.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import TdxStats, check

FEL_NODATA = np.float32(-3.0e38)            # src/flood.cpp:136
P_NODATA = np.int16(-32768)                 # src/d8.cpp:231
SLOPE_NODATA = np.float32(-1.0)             # src/d8.cpp:278
AREA_NODATA = np.float32(-1.0)              # src/aread8.cpp:193
ANG_NODATA = np.float32(-3.402823466e38)    # MISSINGFLOAT, src/commonLib.h:80


DISTDOWN_STATS = {"ave": 0, "max": 1, "min": 2}                    # -m <stat> of src/DinfDistDownmn.cpp:133-196 (and of DinfDistUp)
DISTDOWN_KINDS = {"h": 0, "v": 1, "p": 2, "s": 3}                   # -m <type>


def _distdown_mode(stat, kind):
    if stat not in DISTDOWN_STATS:
        raise ValueError(f"stat must be one of {sorted(DISTDOWN_STATS)}, not {stat!r}")
    if kind not in DISTDOWN_KINDS:
        raise ValueError(f"kind must be one of {sorted(DISTDOWN_KINDS)}, not {kind!r}")
    return DISTDOWN_STATS[stat], DISTDOWN_KINDS[kind]


def _is_torch(x):
    return x is not None and type(x).__module__.startswith("torch")


def _f64(a, n):
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)))
    return a


class Context:
    """Owns a HIP stream, a scratch arena and timing events on one device."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.tdx_context_create(int(device), C.byref(h)))
        self._h = h
        self._owned = True
        self.device = int(device)

    @classmethod
    def borrow(cls, handle, device: int):
        """A Context over a tdx_context* that somebody else owns (a rank of a tdx_group: taudem_amd.distributed.StripGroup)."""
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self._h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        self._owned = False
        self.device = int(device)
        return self

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_owned", True):
                self._lib.tdx_context_destroy(self._h)
            self._h = None

    def release_scratch(self):
        """Frees the scratch arena (it grows again on demand)."""
        check(self._lib.tdx_context_release_scratch(self._h), self._h)

    def set_option(self, name: str, value: int):
        """Context options of include/taudem_amd.h (e.g. "kernel_timing")."""
        check(self._lib.tdx_context_set_option(self._h, name.encode(), int(value)), self._h)

    def segments(self):
        """The segment trace since the last call (option "segment_trace"): [(stage, phase, kind, device_ms, wall_ms)], kind 0 = ended by a halo
        exchange, 1 = by an all-reduce, 2 = by the end of the call.  Clears the log."""
        n = int(self._lib.tdx_context_segments(self._h, None, 0))
        if n == 0:
            return []
        buf = (_lib.TdxSegment * n)()
        self._lib.tdx_context_segments(self._h, buf, n)
        return [(b.stage.decode(), b.phase.decode(), int(b.kind), float(b.device_ms), float(b.wall_ms)) for b in buf]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- helpers --------------------------------------------------------------------------
    def _ptr(self, a, dtype, shape=None, name="array"):
        """(pointer, is_device) for a numpy array or torch cuda tensor; validates dtype/contiguity."""
        if a is None:
            return None, None
        if _is_torch(a):
            import torch

            want = {np.float32: torch.float32, np.int16: torch.int16, np.int32: torch.int32}[dtype]
            if not a.is_cuda or a.device.index != self.device:
                raise ValueError(f"{name}: tensor must live on cuda:{self.device}")
            if a.dtype != want or not a.is_contiguous():
                raise ValueError(f"{name}: need contiguous {want}")
            if shape is not None and tuple(a.shape) != tuple(shape):
                raise ValueError(f"{name}: shape {tuple(a.shape)} != {tuple(shape)}")
            return C.c_void_p(a.data_ptr()), True
        if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous:
            raise ValueError(f"{name}: need C-contiguous numpy {np.dtype(dtype)}")
        if shape is not None and tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(a.shape)} != {tuple(shape)}")
        return C.c_void_p(a.ctypes.data), False

    def _out(self, like, dtype, shape):
        if _is_torch(like):
            import torch

            td = {np.float32: torch.float32, np.int16: torch.int16, np.int32: torch.int32}[dtype]
            return torch.empty(shape, dtype=td, device=like.device)
        return np.empty(shape, dtype=dtype)

    def _sync_torch(self, *arrs):
        if any(_is_torch(a) for a in arrs):
            import torch

            torch.cuda.synchronize(self.device)

    @staticmethod
    def _outlets(outlets):
        if outlets is None:
            return None, None, -1, ()
        ox = np.ascontiguousarray(np.asarray(outlets[0], dtype=np.int32))
        oy = np.ascontiguousarray(np.asarray(outlets[1], dtype=np.int32))
        if ox.shape != oy.shape or ox.ndim != 1:
            raise ValueError("outlets: need two equal-length 1-D index arrays (columns, rows)")
        return C.c_void_p(ox.ctypes.data), C.c_void_p(oy.ctypes.data), int(ox.size), (ox, oy)

    def _pick(self, dev, name):
        return getattr(self._lib, name + ("_dev" if dev else ""))

    # ---- stages ---------------------------------------------------------------------------
    def pitremove(self, dem, nodata=-9999.0, mask=None, fourway=False, out=None, stats=False):
        """fel = flood(dem)  (src/flood.cpp:50)."""
        ny, nx = dem.shape
        fel = out if out is not None else self._out(dem, np.float32, (ny, nx))
        pz, dev = self._ptr(dem, np.float32, name="dem")
        pm, mdev = self._ptr(mask, np.int16, (ny, nx), "mask")
        pf, fdev = self._ptr(fel, np.float32, (ny, nx), "fel")
        if fdev != dev or (mask is not None and mdev != dev):
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(dem, mask)
        check(self._pick(dev, "tdx_pitremove")(self._h, pz, nx, ny, float(nodata), pm, int(bool(fourway)), pf, C.byref(st)), self._h)
        return (fel, st.as_dict()) if stats else fel

    def d8flowdir(self, fel, nodata=float(FEL_NODATA), dx=1.0, dy=1.0, want_slope=True, out=None, stats=False):
        """p, sd8 = setdird8(fel)  (src/d8.cpp:181).  dx, dy: scalars or per-row arrays (metres)."""
        ny, nx = fel.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        p = out[0] if out is not None else self._out(fel, np.int16, (ny, nx))
        sd8 = (out[1] if out is not None else self._out(fel, np.float32, (ny, nx))) if want_slope else None
        pz, dev = self._ptr(fel, np.float32, name="fel")
        pp, pdev = self._ptr(p, np.int16, (ny, nx), "p")
        ps, _ = self._ptr(sd8, np.float32, (ny, nx), "sd8")
        if pdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(fel)
        check(self._pick(dev, "tdx_d8flowdir")(self._h, pz, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data),
                                                pp, ps, C.byref(st)), self._h)
        res = (p, sd8) if want_slope else (p, None)
        return (res + (st.as_dict(),)) if stats else res

    def aread8(self, p, nodata=int(P_NODATA), weights=None, weights_nodata=-9999.0, contcheck=True, outlets=None, out=None, stats=False):
        """ad8 = aread8(p)  (src/aread8.cpp:56).  outlets: (columns, rows) global indices or None."""
        ny, nx = p.shape
        ad8 = out if out is not None else self._out(p, np.float32, (ny, nx))
        pp, dev = self._ptr(p, np.int16, name="p")
        pw, wdev = self._ptr(weights, np.float32, (ny, nx), "weights")
        pa, adev = self._ptr(ad8, np.float32, (ny, nx), "ad8")
        if adev != dev or (weights is not None and wdev != dev):
            raise ValueError("all rasters must be on the same side (host or device)")
        ox, oy, no, keep = self._outlets(outlets)
        st = TdxStats()
        self._sync_torch(p, weights)
        check(self._pick(dev, "tdx_aread8")(self._h, pp, nx, ny, int(nodata), pw, float(weights_nodata), int(bool(contcheck)), ox, oy, no, pa,
                                             C.byref(st)), self._h)
        del keep
        return (ad8, st.as_dict()) if stats else ad8

    def d8flowpathextremeup(self, p, sa, nodata=int(P_NODATA), usemax=True, contcheck=True, outlets=None, out=None, stats=False):
        """ssa = d8flowpathextremeup(p, sa)  (src/D8flowpathextremeup.cpp:58): upstream max / min of sa along D8 flow paths (nodata -FLT_MAX)."""
        ny, nx = p.shape
        ssa = out if out is not None else self._out(p, np.float32, (ny, nx))
        pp, dev = self._ptr(p, np.int16, name="p")
        pa, adev = self._ptr(sa, np.float32, (ny, nx), "sa")
        ps, sdev = self._ptr(ssa, np.float32, (ny, nx), "ssa")
        if adev != dev or sdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        ox, oy, no, keep = self._outlets(outlets)
        st = TdxStats()
        self._sync_torch(p, sa)
        check(self._pick(dev, "tdx_d8flowpathextremeup")(self._h, pp, nx, ny, int(nodata), pa, int(bool(usemax)), int(bool(contcheck)), ox, oy, no, ps,
                                                          C.byref(st)), self._h)
        del keep
        return (ssa, st.as_dict()) if stats else ssa

    def gridnet(self, p, nodata=int(P_NODATA), dx=1.0, dy=1.0, mask=None, thresh=0, outlets=None, stats=False):
        """plen, tlen, gord = gridnet(p)  (src/gridnet.cpp:54).  mask: int32 raster, cells with mask >= thresh are evaluated;
        outlets: (columns, rows) - only their upstream closure is evaluated."""
        ny, nx = p.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        plen = self._out(p, np.float32, (ny, nx))
        tlen = self._out(p, np.float32, (ny, nx))
        gord = self._out(p, np.int16, (ny, nx))
        pp, dev = self._ptr(p, np.int16, name="p")
        pm, mdev = self._ptr(mask, np.int32, (ny, nx), "mask")
        ppl, _ = self._ptr(plen, np.float32, (ny, nx), "plen")
        ptl, _ = self._ptr(tlen, np.float32, (ny, nx), "tlen")
        pgo, _ = self._ptr(gord, np.int16, (ny, nx), "gord")
        if mask is not None and mdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        ox, oy, no, keep = self._outlets(outlets)
        self._sync_torch(p, mask)
        check(self._pick(dev, "tdx_gridnet")(self._h, pp, nx, ny, int(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data), pm, int(thresh),
                                              ox, oy, no, ppl, ptl, pgo, C.byref(st)), self._h)
        del keep
        return (plen, tlen, gord, st.as_dict()) if stats else (plen, tlen, gord)

    def threshold(self, ssa, thresh, nodata=-1.0, mask=None, stats=False):
        """src = threshold(ssa)  (src/Threshold.cpp:49): 1 where ssa >= thresh (and mask >= 0), 0 elsewhere, -32768 where ssa is nodata."""
        ny, nx = ssa.shape
        src = self._out(ssa, np.int16, (ny, nx))
        pa, dev = self._ptr(ssa, np.float32, name="ssa")
        pm, mdev = self._ptr(mask, np.float32, (ny, nx), "mask")
        ps, _ = self._ptr(src, np.int16, (ny, nx), "src")
        if mask is not None and mdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(ssa, mask)
        check(self._pick(dev, "tdx_threshold")(self._h, pa, nx, ny, float(nodata), pm, float(thresh), ps, C.byref(st)), self._h)
        return (src, st.as_dict()) if stats else src

    def dinfflowdir(self, fel, nodata=float(FEL_NODATA), dx=1.0, dy=1.0, out=None, stats=False):
        """ang, slp = setdir(fel)  (src/dinf.cpp:109)."""
        ny, nx = fel.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        ang = out[0] if out is not None else self._out(fel, np.float32, (ny, nx))
        slp = out[1] if out is not None else self._out(fel, np.float32, (ny, nx))
        pz, dev = self._ptr(fel, np.float32, name="fel")
        pa, adev = self._ptr(ang, np.float32, (ny, nx), "ang")
        ps, _ = self._ptr(slp, np.float32, (ny, nx), "slp")
        if adev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(fel)
        check(self._pick(dev, "tdx_dinfflowdir")(self._h, pz, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data),
                                                  pa, ps, C.byref(st)), self._h)
        return (ang, slp, st.as_dict()) if stats else (ang, slp)

    def areadinf(self, ang, nodata=float(ANG_NODATA), dx=1.0, dy=1.0, weights=None, contcheck=True, outlets=None, out=None, stats=False):
        """sca = area(ang)  (src/areadinf.cpp:53)."""
        ny, nx = ang.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        sca = out if out is not None else self._out(ang, np.float32, (ny, nx))
        pa, dev = self._ptr(ang, np.float32, name="ang")
        pw, wdev = self._ptr(weights, np.float32, (ny, nx), "weights")
        ps, sdev = self._ptr(sca, np.float32, (ny, nx), "sca")
        if sdev != dev or (weights is not None and wdev != dev):
            raise ValueError("all rasters must be on the same side (host or device)")
        ox, oy, no, keep = self._outlets(outlets)
        st = TdxStats()
        self._sync_torch(ang, weights)
        check(self._pick(dev, "tdx_areadinf")(self._h, pa, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data), pw,
                                               int(bool(contcheck)), ox, oy, no, ps, C.byref(st)), self._h)
        del keep
        return (sca, st.as_dict()) if stats else sca

    def dinfdecayaccum(self, ang, dm, nodata=float(ANG_NODATA), dm_nodata=-9999.0, dx=1.0, dy=1.0, weights=None, contcheck=True,
                       outlets=None, out=None, stats=False):
        """dsca = dmarea(ang, dm)  (src/dinfdecayaccum.cpp:61)."""
        ny, nx = ang.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        dsca = out if out is not None else self._out(ang, np.float32, (ny, nx))
        pa, dev = self._ptr(ang, np.float32, name="ang")
        pd, ddev = self._ptr(dm, np.float32, (ny, nx), "dm")
        pw, wdev = self._ptr(weights, np.float32, (ny, nx), "weights")
        ps, sdev = self._ptr(dsca, np.float32, (ny, nx), "dsca")
        if sdev != dev or ddev != dev or (weights is not None and wdev != dev):
            raise ValueError("all rasters must be on the same side (host or device)")
        ox, oy, no, keep = self._outlets(outlets)
        st = TdxStats()
        self._sync_torch(ang, dm, weights)
        check(self._pick(dev, "tdx_dinfdecayaccum")(self._h, pa, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data),
                                                     pd, float(dm_nodata), pw, int(bool(contcheck)), ox, oy, no, ps, C.byref(st)), self._h)
        del keep
        return (dsca, st.as_dict()) if stats else dsca

    def dinfupdependence(self, ang, dg, nodata=float(ANG_NODATA), dx=1.0, dy=1.0, stats=False):
        """dep = depgrd(ang, dg)  (src/DinfUpDependence.cpp:52): dg int32, dep float32 (nodata -1)."""
        ny, nx = ang.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        dep = self._out(ang, np.float32, (ny, nx))
        pa, dev = self._ptr(ang, np.float32, name="ang")
        pg, gdev = self._ptr(dg, np.int32, (ny, nx), "dg")
        po, _ = self._ptr(dep, np.float32, (ny, nx), "dep")
        if gdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(ang, dg)
        check(self._pick(dev, "tdx_dinfupdependence")(self._h, pa, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data), pg, po,
                                                       C.byref(st)), self._h)
        return (dep, st.as_dict()) if stats else dep

    def dinfrevaccum(self, ang, w, nodata=float(ANG_NODATA), w_nodata=-9999.0, dx=1.0, dy=1.0, stats=False):
        """racc, dmax = dsaccum(ang, w)  (src/DinfRevAccum.cpp:51): float32, nodata -FLT_MAX."""
        ny, nx = ang.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        racc = self._out(ang, np.float32, (ny, nx))
        dmax = self._out(ang, np.float32, (ny, nx))
        pa, dev = self._ptr(ang, np.float32, name="ang")
        pw, wdev = self._ptr(w, np.float32, (ny, nx), "w")
        pr, _ = self._ptr(racc, np.float32, (ny, nx), "racc")
        pm, _ = self._ptr(dmax, np.float32, (ny, nx), "dmax")
        if wdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(ang, w)
        check(self._pick(dev, "tdx_dinfrevaccum")(self._h, pa, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data), pw,
                                                   float(w_nodata), pr, pm, C.byref(st)), self._h)
        return (racc, dmax, st.as_dict()) if stats else (racc, dmax)

    def dinfdistdown(self, ang, src, fel=None, *, stat="ave", kind="v", weights=None, weights_nodata=-9999.0, contcheck=True, dx=1.0, dy=1.0,
                     nodata=float(ANG_NODATA), fel_nodata=float(FEL_NODATA), stats=False):
        """dd = dinfdistdown(ang, fel, src, w)  (src/DinfDistDown.cpp:66): distance from each cell down to the stream (src int16 >= 1).

        kind "h" horizontal, "v" vertical drop (with stat "ave": HAND), "p" Pythagorean, "s" surface; stat "ave", "max" or "min" over
        the receivers.  `fel` is required for v, p and s; `weights` scale the horizontal steps of h, p and s (v ignores them, as the
        reference does).  dd float32, nodata -FLT_MAX."""
        sm, tm = _distdown_mode(stat, kind)
        if tm != DISTDOWN_KINDS["h"] and fel is None:
            raise ValueError(f"kind {kind!r} needs fel")
        ny, nx = ang.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        dd = self._out(ang, np.float32, (ny, nx))
        use_fel = tm != DISTDOWN_KINDS["h"]
        use_w = weights is not None and tm != DISTDOWN_KINDS["v"]
        pa, dev = self._ptr(ang, np.float32, name="ang")
        ps, sdev = self._ptr(src, np.int16, (ny, nx), "src")
        pf, fdev = self._ptr(fel if use_fel else None, np.float32, (ny, nx), "fel")
        pw, wdev = self._ptr(weights if use_w else None, np.float32, (ny, nx), "weights")
        po, _ = self._ptr(dd, np.float32, (ny, nx), "dd")
        if sdev != dev or (use_fel and fdev != dev) or (use_w and wdev != dev):
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(ang, src, fel, weights)
        check(self._pick(dev, "tdx_dinfdistdown")(self._h, pa, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data), pf,
                                                   float(fel_nodata), ps, pw, float(weights_nodata), sm, tm, int(bool(contcheck)), po, C.byref(st)), self._h)
        return (dd, st.as_dict()) if stats else dd

    def d8hdisttostrm(self, p, src, thresh=1, *, dx=1.0, dy=1.0, nodata=int(P_NODATA), src_nodata=-2147483647, stats=False):
        """dist = distgrid(p, src)  (src/D8HDistToStrm.cpp:57): horizontal distance along the D8 flow path down to the stream.

        Stream cells are those where src (int32, the reference's LONG read) is not src_nodata and is >= thresh, whatever p is there;
        they get 0.  dist float32, nodata -FLT_MAX (off the raster, into a cell without a result, around a cycle)."""
        ny, nx = p.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        dist = self._out(p, np.float32, (ny, nx))
        pp, dev = self._ptr(p, np.int16, name="p")
        ps, sdev = self._ptr(src, np.int32, (ny, nx), "src")
        po, _ = self._ptr(dist, np.float32, (ny, nx), "dist")
        if sdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(p, src)
        check(self._pick(dev, "tdx_d8hdisttostrm")(self._h, pp, nx, ny, int(nodata), ps, int(src_nodata), int(thresh), C.c_void_p(dxc.ctypes.data),
                                                   C.c_void_p(dyc.ctypes.data), po, C.byref(st)), self._h)
        return (dist, st.as_dict()) if stats else dist

    def d8vdisttostrm(self, p, fel, src, thresh=1, *, nodata=int(P_NODATA), src_nodata=-2147483647, stats=False):
        """dist = d8vdistdown(p, fel, src)  (src/D8VDistToStrm.cpp:58): vertical drop along the D8 flow path down to the stream.

        Stream cells as for d8hdisttostrm; every other cell gets (fel - fel(receiver)) + dist(receiver) in float32.  fel is read with no
        nodata test, as in the reference.  dist float32, nodata -FLT_MAX."""
        ny, nx = p.shape
        dist = self._out(p, np.float32, (ny, nx))
        pp, dev = self._ptr(p, np.int16, name="p")
        pf, fdev = self._ptr(fel, np.float32, (ny, nx), "fel")
        ps, sdev = self._ptr(src, np.int32, (ny, nx), "src")
        po, _ = self._ptr(dist, np.float32, (ny, nx), "dist")
        if sdev != dev or fdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(p, fel, src)
        check(self._pick(dev, "tdx_d8vdisttostrm")(self._h, pp, nx, ny, int(nodata), pf, ps, int(src_nodata), int(thresh), po, C.byref(st)), self._h)
        return (dist, st.as_dict()) if stats else dist

    def flowdircond(self, p, z, *, nodata=int(P_NODATA), z_nodata=float(FEL_NODATA), stats=False):
        """zfdc = flowdircond(p, z)  (src/flowdircond.cpp:54): z conditioned along the D8 directions - from the ridges downstream every
        cell becomes the minimum of its own z and the conditioned z of the cells that drain into it.

        Cells the reference's queue never reaches (no valid direction, below a p == 0 cell, on or below a cycle) and cells with nodata z
        keep their input value; the result carries z's nodata value."""
        ny, nx = p.shape
        out = self._out(p, np.float32, (ny, nx))
        pp, dev = self._ptr(p, np.int16, name="p")
        pz, zdev = self._ptr(z, np.float32, (ny, nx), "z")
        po, _ = self._ptr(out, np.float32, (ny, nx), "zfdc")
        if zdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(p, z)
        check(self._pick(dev, "tdx_flowdircond")(self._h, pp, nx, ny, int(nodata), pz, float(z_nodata), po, C.byref(st)), self._h)
        return (out, st.as_dict()) if stats else out

    def slopeavedown(self, p, fel, dn=50.0, *, dx=1.0, dy=1.0, niter=None, nodata=int(P_NODATA), fel_nodata=float(FEL_NODATA), stats=False):
        """slpd = sloped(p, fel, dn)  (src/SlopeAveDown.cpp:59): the slope from each cell to the cell the distance dn down its D8 flow path.

        niter (default int(dn / min(dx, dy) of the middle row) + 1, the reference's count; not capped) synchronous one-step pulls along
        the D8 pointer.  dn must be finite and not negative.  slpd float32, nodata -FLT_MAX."""
        ny, nx = p.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        out = self._out(p, np.float32, (ny, nx))
        pp, dev = self._ptr(p, np.int16, name="p")
        pf, fdev = self._ptr(fel, np.float32, (ny, nx), "fel")
        po, _ = self._ptr(out, np.float32, (ny, nx), "slpd")
        if fdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(p, fel)
        check(self._pick(dev, "tdx_slopeavedown")(self._h, pp, nx, ny, int(nodata), pf, float(fel_nodata), C.c_void_p(dxc.ctypes.data),
                                                  C.c_void_p(dyc.ctypes.data), float(dn), int(niter) if niter else 0, po, C.byref(st)), self._h)
        return (out, st.as_dict()) if stats else out

    def catchhydrogeo(self, hand, catch, slp, ids, stages, *, dx=1.0, dy=1.0, hand_nodata=float(ANG_NODATA), catch_nodata=-9999, slp_nodata=-1.0, stats=False):
        """count, surface, bed, volume, catcharea = catchhydrogeo(hand, catch, slp, ids, stages)  (src/CatchHydroGeo.cpp:69).

        Per listed catchment id and stage: the cells of the catchment whose hand is below the stage (or within 1e-6 of 0), their plan area,
        bed area and volume; and each catchment's whole plan area.  ids: int32 list (the last row of a repeated id wins, earlier rows stay 0);
        stages: float64, any order.  count int32 and surface / bed / volume float64 are [len(stages)][len(ids)], catcharea float64 [len(ids)];
        all numpy arrays on the host.  The fp64 sums are taken in a fixed order: the same input gives the same bits."""
        ny, nx = hand.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32)).reshape(-1)
        stages = np.ascontiguousarray(np.asarray(stages, dtype=np.float64)).reshape(-1)
        nc, nh = ids.size, stages.size
        ph, dev = self._ptr(hand, np.float32, name="hand")
        pc, cdev = self._ptr(catch, np.int32, (ny, nx), "catch")
        ps, sdev = self._ptr(slp, np.float32, (ny, nx), "slp")
        if cdev != dev or sdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        count = np.zeros((nh, nc), np.int32)
        surface, bed, volume = (np.zeros((nh, nc), np.float64) for _ in range(3))
        catcharea = np.zeros(nc, np.float64)
        st = TdxStats()
        self._sync_torch(hand, catch, slp)
        v = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        check(self._pick(dev, "tdx_catchhydrogeo")(self._h, ph, pc, ps, nx, ny, float(hand_nodata), int(catch_nodata), float(slp_nodata), v(dxc), v(dyc), v(ids), nc,
                                                   v(stages), nh, v(count), v(surface), v(bed), v(volume), v(catcharea), C.byref(st)), self._h)
        res = (count, surface, bed, volume, catcharea)
        return res + (st.as_dict(),) if stats else res

    def inundepth(self, hand, catch, ids, depth, *, mask=None, area=True, dx=1.0, dy=1.0, hand_nodata=float(ANG_NODATA), catch_nodata=-9999, mask_nodata=-32768,
                  stats=False):
        """map, area = inundepth(hand, catch, ids, depth)  (src/InunDepth.cpp:53, the raster part).

        ids / depth: one forecast depth (float32) per id, the last row of a repeated id wins.  map float32, nodata -3.0e38: depth - hand where
        catch and hand have data, depth >= 0 and depth > hand + 0.001.  mask (int16): as in the reference, with a mask every cell of the map is
        nodata.  area (float32 per row, None with area=False): plan area of the cells with depth > 0 and depth - hand > 0, at the winning row
        of each id, 0 elsewhere; summed in fp64 and rounded once."""
        ny, nx = hand.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32)).reshape(-1)
        depth = np.ascontiguousarray(np.asarray(depth, dtype=np.float32)).reshape(-1)
        if ids.size != depth.size:
            raise ValueError("ids and depth: need equal lengths")
        out = self._out(hand, np.float32, (ny, nx))
        ph, dev = self._ptr(hand, np.float32, name="hand")
        pc, cdev = self._ptr(catch, np.int32, (ny, nx), "catch")
        pm, mdev = self._ptr(mask, np.int16, (ny, nx), "mask")
        po, _ = self._ptr(out, np.float32, (ny, nx), "map")
        if cdev != dev or (mask is not None and mdev != dev):
            raise ValueError("all rasters must be on the same side (host or device)")
        wet = np.zeros(ids.size, np.float32) if area else None
        st = TdxStats()
        self._sync_torch(hand, catch, mask)
        v = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        check(self._pick(dev, "tdx_inundepth")(self._h, ph, pc, pm, nx, ny, float(hand_nodata), int(catch_nodata), int(mask_nodata), v(dxc), v(dyc), v(ids), v(depth),
                                               ids.size, po, v(wet) if area else None, C.byref(st)), self._h)
        return (out, wet, st.as_dict()) if stats else (out, wet)

    def gagewatershed(self, p, outlets, *, nodata=int(P_NODATA), stats=False):
        """gw, id_table = gagewatershed(p, outlets)  (src/gagewatershed.cpp:56): every cell gets the id of the first gauge downstream of it.

        outlets: (columns, rows[, ids]) global indices (ids default to 1..n, as the outlet reader's); outlets off the raster are skipped and
        the first one on a cell wins.  gw int32, nodata -2147483647.  id_table: int32 array (k, 2) of the `-id` file's lines (id, iddown)
        for the k placed outlets in input order; iddown is -1 where the gauge's downstream neighbour is off the raster or unlabelled."""
        ny, nx = p.shape
        ox = np.ascontiguousarray(np.asarray(outlets[0], dtype=np.int32)).reshape(-1)
        oy = np.ascontiguousarray(np.asarray(outlets[1], dtype=np.int32)).reshape(-1)
        ids = np.arange(1, ox.size + 1, dtype=np.int32) if len(outlets) < 3 else np.ascontiguousarray(np.asarray(outlets[2], dtype=np.int32)).reshape(-1)
        if ox.shape != oy.shape or ox.shape != ids.shape:
            raise ValueError("outlets: need equal-length 1-D arrays (columns, rows[, ids])")
        gw = self._out(p, np.int32, (ny, nx))
        pp, dev = self._ptr(p, np.int16, name="p")
        pg, _ = self._ptr(gw, np.int32, (ny, nx), "gw")
        placed = np.zeros(ox.size + 1, np.int32)
        iddown = np.zeros(ox.size + 1, np.int32)
        st = TdxStats()
        self._sync_torch(p)
        check(self._pick(dev, "tdx_gagewatershed")(self._h, pp, nx, ny, int(nodata), C.c_void_p(ox.ctypes.data), C.c_void_p(oy.ctypes.data),
                                                   C.c_void_p(ids.ctypes.data), int(ox.size), pg, C.c_void_p(placed.ctypes.data),
                                                   C.c_void_p(iddown.ctypes.data), C.byref(st)), self._h)
        keep = placed[:ox.size] > 0
        table = np.stack([ids[keep], iddown[:ox.size][keep]], axis=1).astype(np.int32)
        return (gw, table, st.as_dict()) if stats else (gw, table)

    def dinfdistup(self, ang, fel=None, *, stat="ave", kind="h", weights=None, weights_nodata=-9999.0, contcheck=True, thresh=0.0, dx=1.0, dy=1.0,
                   nodata=float(ANG_NODATA), fel_nodata=float(FEL_NODATA), stats=False):
        """du = dinfdistup(ang, fel, w)  (src/DinfDistUp.cpp:65): distance from each cell up to the ridge over the neighbours that drain into it.

        kind "h" horizontal, "v" vertical rise, "p" Pythagorean, "s" surface; stat "ave", "max" or "min" over the contributors; a
        neighbour contributes only if its proportion exceeds `thresh`.  `fel` is required for v, p and s; `weights` scale the horizontal
        steps of h, p and s (v ignores them, as the reference does).  du float32, nodata -FLT_MAX; ridge cells get 0."""
        sm, tm = _distdown_mode(stat, kind)
        if tm != DISTDOWN_KINDS["h"] and fel is None:
            raise ValueError(f"kind {kind!r} needs fel")
        ny, nx = ang.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        du = self._out(ang, np.float32, (ny, nx))
        use_fel = tm != DISTDOWN_KINDS["h"]
        use_w = weights is not None and tm != DISTDOWN_KINDS["v"]
        pa, dev = self._ptr(ang, np.float32, name="ang")
        pf, fdev = self._ptr(fel if use_fel else None, np.float32, (ny, nx), "fel")
        pw, wdev = self._ptr(weights if use_w else None, np.float32, (ny, nx), "weights")
        po, _ = self._ptr(du, np.float32, (ny, nx), "du")
        if (use_fel and fdev != dev) or (use_w and wdev != dev):
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(ang, fel, weights)
        check(self._pick(dev, "tdx_dinfdistup")(self._h, pa, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data), pf,
                                                 float(fel_nodata), pw, float(weights_nodata), sm, tm, int(bool(contcheck)), float(thresh), po,
                                                 C.byref(st)), self._h)
        return (du, st.as_dict()) if stats else du

    def retlimflow(self, ang, wg, rc, *, dx=1.0, dy=1.0, nodata=float(ANG_NODATA), wg_nodata=-9999.0, rc_nodata=-9999.0, stats=False):
        """qrl = retlimro(ang, wg, rc)  (src/RetlimFlow.cpp:53): retention limited runoff, max(0, inflow + wg - rc) accumulated along the
        D-infinity flow.  A cell whose wg or rc is nodata has no value, and neither has anything downstream of it.  qrl float32, nodata -FLT_MAX."""
        ny, nx = ang.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        qrl = self._out(ang, np.float32, (ny, nx))
        pa, dev = self._ptr(ang, np.float32, name="ang")
        pw, wdev = self._ptr(wg, np.float32, (ny, nx), "wg")
        pr, rdev = self._ptr(rc, np.float32, (ny, nx), "rc")
        po, _ = self._ptr(qrl, np.float32, (ny, nx), "qrl")
        if wdev != dev or rdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        st = TdxStats()
        self._sync_torch(ang, wg, rc)
        check(self._pick(dev, "tdx_retlimflow")(self._h, pa, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data), pw, float(wg_nodata), pr,
                                                 float(rc_nodata), po, C.byref(st)), self._h)
        return (qrl, st.as_dict()) if stats else qrl

    def dinfavalanche(self, ang, fel, ass, *, thresh=0.2, alpha=18.0, direct=False, dx=1.0, dy=1.0, geo=None, geographic=False, nodata=float(ANG_NODATA),
                      fel_nodata=float(FEL_NODATA), ass_nodata=-32768, stats=False):
        """rz, dfs = avalancherunoutgrd(ang, fel, ass)  (src/DinfAvalanche.cpp:62): the runout zone below the source cells (ass > 0, int16) as the
        angle to the source in degrees, and the distance from the source - along the flow path, or with direct=True as a straight line in
        the raster's coordinates: geo = (xleftedge, ytopedge, dlon, dlat), by default (0, ny * dy[0], dx[0], dy[0]); needed when
        geographic, where dlon / dlat are degrees.  float32, nodata -FLT_MAX."""
        ny, nx = ang.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        rz = self._out(ang, np.float32, (ny, nx))
        dfs = self._out(ang, np.float32, (ny, nx))
        pa, dev = self._ptr(ang, np.float32, name="ang")
        pf, fdev = self._ptr(fel, np.float32, (ny, nx), "fel")
        ps, sdev = self._ptr(ass, np.int16, (ny, nx), "ass")
        pz, _ = self._ptr(rz, np.float32, (ny, nx), "rz")
        pd, _ = self._ptr(dfs, np.float32, (ny, nx), "dfs")
        if fdev != dev or sdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        g4 = None if geo is None else np.ascontiguousarray(np.asarray(geo, dtype=np.float64).reshape(4))
        st = TdxStats()
        self._sync_torch(ang, fel, ass)
        check(self._pick(dev, "tdx_dinfavalanche")(self._h, pa, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data), pf, float(fel_nodata),
                                                    ps, int(ass_nodata), float(thresh), float(alpha), 0 if direct else 1,
                                                    None if g4 is None else C.c_void_p(g4.ctypes.data), int(bool(geographic)), pz, pd, C.byref(st)), self._h)
        return (rz, dfs, st.as_dict()) if stats else (rz, dfs)

    def dinfconclimaccum(self, ang, dm, dg, q, csol=1.0, nodata=float(ANG_NODATA), dm_nodata=-9999.0, q_nodata=-9999.0, dx=1.0, dy=1.0, contcheck=True,
                         outlets=None, stats=False):
        """ctpt = dsllArea(ang, dm, dg, q)  (src/DinfConcLimAccum.cpp:61): dg int16, ctpt float32 (nodata -FLT_MAX)."""
        ny, nx = ang.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        ctpt = self._out(ang, np.float32, (ny, nx))
        pa, dev = self._ptr(ang, np.float32, name="ang")
        pm, mdev = self._ptr(dm, np.float32, (ny, nx), "dm")
        pg, gdev = self._ptr(dg, np.int16, (ny, nx), "dg")
        pq, qdev = self._ptr(q, np.float32, (ny, nx), "q")
        po, _ = self._ptr(ctpt, np.float32, (ny, nx), "ctpt")
        if mdev != dev or gdev != dev or qdev != dev:
            raise ValueError("all rasters must be on the same side (host or device)")
        ox, oy, no, keep = self._outlets(outlets)
        st = TdxStats()
        self._sync_torch(ang, dm, dg, q)
        check(self._pick(dev, "tdx_dinfconclimaccum")(self._h, pa, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data), pm, float(dm_nodata),
                                                       pg, pq, float(q_nodata), float(csol), int(bool(contcheck)), ox, oy, no, po, C.byref(st)), self._h)
        del keep
        return (ctpt, st.as_dict()) if stats else ctpt

    def dinftranslimaccum(self, ang, tsup, tc, cs=None, nodata=float(ANG_NODATA), tsup_nodata=-9999.0, tc_nodata=-9999.0, cs_nodata=-9999.0, dx=1.0, dy=1.0,
                          contcheck=True, outlets=None, stats=False):
        """tla, tdep, ctpt = tlaccum(ang, tsup, tc[, cs])  (src/DinfTransLimAccum.cpp:61): float32, nodata -FLT_MAX; ctpt is None without cs."""
        ny, nx = ang.shape
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        tla = self._out(ang, np.float32, (ny, nx))
        dep = self._out(ang, np.float32, (ny, nx))
        cso = self._out(ang, np.float32, (ny, nx)) if cs is not None else None
        pa, dev = self._ptr(ang, np.float32, name="ang")
        ps, sdev = self._ptr(tsup, np.float32, (ny, nx), "tsup")
        pc, cdev = self._ptr(tc, np.float32, (ny, nx), "tc")
        pi, idev = self._ptr(cs, np.float32, (ny, nx), "cs")
        pt, _ = self._ptr(tla, np.float32, (ny, nx), "tla")
        pd, _ = self._ptr(dep, np.float32, (ny, nx), "tdep")
        po, _ = self._ptr(cso, np.float32, (ny, nx), "ctpt")
        if sdev != dev or cdev != dev or (cs is not None and idev != dev):
            raise ValueError("all rasters must be on the same side (host or device)")
        ox, oy, no, keep = self._outlets(outlets)
        st = TdxStats()
        self._sync_torch(ang, tsup, tc, cs)
        check(self._pick(dev, "tdx_dinftranslimaccum")(self._h, pa, nx, ny, float(nodata), C.c_void_p(dxc.ctypes.data), C.c_void_p(dyc.ctypes.data), ps,
                                                        float(tsup_nodata), pc, float(tc_nodata), pi, float(cs_nodata), int(bool(contcheck)), ox, oy, no, pt, pd, po,
                                                        C.byref(st)), self._h)
        del keep
        return (tla, dep, cso, st.as_dict()) if stats else (tla, dep, cso)

    def synth_dem(self, n_or_shape, seed=1234, x0=0, y0=0, base_wavelength=None, out=None):
        """Seeded fractal DEM generated on the device (torch tensor on cuda:<device>)."""
        import torch

        if isinstance(n_or_shape, int):
            ny = nx = int(n_or_shape)
        else:
            ny, nx = n_or_shape
        if base_wavelength is None:
            base_wavelength = synth_base_wavelength(max(nx, ny))
        t = out if out is not None else torch.empty((ny, nx), dtype=torch.float32, device=f"cuda:{self.device}")
        torch.cuda.synchronize(self.device)
        check(self._lib.tdx_synth_dem_dev(self._h, int(seed), nx, ny, int(x0), int(y0), int(base_wavelength), C.c_void_p(t.data_ptr())), self._h)
        return t


def catchhydrogeo(hand, catch, slp, ids, stages, device=0, **kw):
    """Context(device).catchhydrogeo(...) for a single call."""
    with Context(device) as ctx:
        return ctx.catchhydrogeo(hand, catch, slp, ids, stages, **kw)


def inundepth(hand, catch, ids, depth, device=0, **kw):
    """Context(device).inundepth(...) for a single call."""
    with Context(device) as ctx:
        return ctx.inundepth(hand, catch, ids, depth, **kw)


def synth_base_wavelength(n: int) -> int:
    """Largest power of two < n (at least 2): tdx_synth_base_wl() of csrc/synth_dem.h."""
    wl = 2
    while wl * 2 < n:
        wl *= 2
    return wl


# ---- raster files ---------------------------------------------------------------------------
_NP2DT = {np.dtype(np.int16): _lib.TDX_DT_I16, np.dtype(np.int32): _lib.TDX_DT_I32, np.dtype(np.float32): _lib.TDX_DT_F32}


def raster_info(path):
    info = _lib.TdxRasterInfo()
    check(_lib.load().tdx_raster_info_read(str(path).encode(), C.byref(info)))
    return {
        "nx": info.nx, "ny": info.ny, "geotransform": tuple(info.geotransform), "nodata": info.nodata,
        "has_nodata": bool(info.has_nodata), "geographic": bool(info.geographic), "dxA": info.dxA, "dyA": info.dyA,
    }


def read_raster(path, dtype=np.float32):
    """Returns (array, info dict incl. per-row 'dxc'/'dyc')."""
    info = raster_info(path)
    a = np.empty((info["ny"], info["nx"]), dtype=dtype)
    dxc = np.empty(info["ny"], dtype=np.float64)
    dyc = np.empty(info["ny"], dtype=np.float64)
    check(_lib.load().tdx_raster_read(str(path).encode(), _NP2DT[np.dtype(dtype)], C.c_void_p(a.ctypes.data), C.c_void_p(dxc.ctypes.data),
                                      C.c_void_p(dyc.ctypes.data)))
    info["dxc"], info["dyc"] = dxc, dyc
    return a, info


def write_raster(path, a, nodata, like=None, geotransform=None, geographic=False, lzw=False):
    a = np.ascontiguousarray(a)
    ny, nx = a.shape
    lib = _lib.load()
    if like is not None:
        check(lib.tdx_raster_write(str(path).encode(), _NP2DT[a.dtype], C.c_void_p(a.ctypes.data), nx, ny, float(nodata), str(like).encode(), int(lzw)))
    else:
        gt = np.asarray(geotransform if geotransform is not None else (0.0, 1.0, 0.0, float(ny), 0.0, -1.0), dtype=np.float64)
        check(lib.tdx_raster_write_geo(str(path).encode(), _NP2DT[a.dtype], C.c_void_p(a.ctypes.data), nx, ny, float(nodata),
                                       C.c_void_p(gt.ctypes.data), int(bool(geographic)), int(lzw)))
