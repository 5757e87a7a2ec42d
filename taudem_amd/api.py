"""In-memory interface to the HIP hot path (one :class:`Context` per GPU / process rank).

Every method accepts either numpy arrays (host buffers: the library stages them over PCIe) or torch
CUDA tensors on the context's device (HBM-resident: no copies, the benchmark path).  Array layout,
dtypes and nodata conventions are the reference's (include/taudem_amd.h).
"""
from __future__ import annotations

import ctypes as C
import os

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


def _distdown_mode(stat, kind, fel, weights):
    """(statmethod, typemethod, fel, weights) of DinfDistDown / DinfDistUp: fel is needed by every kind but "h", which does not read it;
    "v" does not read the weights."""
    if stat not in DISTDOWN_STATS:
        raise ValueError(f"stat must be one of {sorted(DISTDOWN_STATS)}, not {stat!r}")
    if kind not in DISTDOWN_KINDS:
        raise ValueError(f"kind must be one of {sorted(DISTDOWN_KINDS)}, not {kind!r}")
    if kind != "h" and fel is None:
        raise ValueError(f"kind {kind!r} needs fel")
    return DISTDOWN_STATS[stat], DISTDOWN_KINDS[kind], fel if kind != "h" else None, weights if kind != "v" else None


def _is_torch(x):
    return x is not None and type(x).__module__.startswith("torch")


def _f64(a, n):
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)))
    return a


def _flat(a, dtype):
    return np.ascontiguousarray(np.asarray(a, dtype=dtype)).reshape(-1)


def _v(a):
    return C.c_void_p(a.ctypes.data)


def _torch_dtype(dtype):
    import torch

    return {np.float32: torch.float32, np.int16: torch.int16, np.int32: torch.int32}[dtype]


class _Call:
    """The frame of one library call, shared by Context.<tool> and StripPipeline.<tool>.  It registers the rasters under one rule, turns
    cell sizes and outlets into host arrays that live as long as it does, and makes the call: tdx_<tool> for numpy rasters,
    tdx_<tool>_dev for tensors, tdx_<tool>_strip (with the comm after the context) for a strip.

    The rule: every raster is a C-contiguous numpy array or a contiguous CUDA tensor of the dtype asked for; the first one registered
    decides the side (host or device) and, for a Context, the shape (ny, nx); every later one, outputs included, has that side and that
    shape.  A strip takes tensors only, of shape (ny_local + 2, nx).  Anything else raises ValueError before the library is entered."""

    def __init__(self, ctx, strip_shape=None, comm=None):
        self.ctx, self.strip, self.shape, self.comm = ctx, strip_shape is not None, strip_shape, comm
        self.first = None      # the first raster: the side, and what outputs are allocated like
        self.keep = []         # host arrays the library reads through the bare pointers handed out

    def raster(self, a, dtype, name):
        """The pointer of raster `a` (None for None, an optional raster not given) after the checks of the rule."""
        if a is None:
            return None
        dev = _is_torch(a)
        if dev:
            if not a.is_cuda or (not self.strip and a.device.index != self.ctx.device):
                raise ValueError(f"{name}: tensor must live on cuda:{self.ctx.device}")
            if a.dtype != _torch_dtype(dtype) or not a.is_contiguous():
                raise ValueError(f"{name}: need contiguous {_torch_dtype(dtype)}")
        elif self.strip:
            raise ValueError(f"{name}: a strip array is a CUDA tensor")
        elif not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous:
            raise ValueError(f"{name}: need C-contiguous numpy {np.dtype(dtype)}")
        if self.first is None:
            if self.shape is None:
                ny, nx = a.shape
                self.shape = (ny, nx)
            self.first, self.dev = a, dev
            self.rows, self.nx = self.shape                       # rows of the array in hand: what dx / dy are broadcast over
            self.ny = self.rows - 2 if self.strip else self.rows   # what the library is told: a strip's owned rows
        if dev != self.dev:
            raise ValueError(f"{name}: all rasters must be on the same side (host or device)")
        if tuple(a.shape) != tuple(self.shape):
            raise ValueError(f"{name}: shape {tuple(a.shape)} != {tuple(self.shape)}")
        return C.c_void_p(a.data_ptr() if dev else a.ctypes.data)

    def out(self, given, dtype, name):
        """(raster, pointer) of an output: the caller's out= if given, else a new one like the first raster."""
        if given is not None:
            a = given
        elif self.dev:
            import torch

            a = torch.empty(self.shape, dtype=_torch_dtype(dtype), device=self.first.device)
        else:
            a = np.empty(self.shape, dtype=dtype)
        return a, self.raster(a, dtype, name)

    def cells(self, dx, dy):
        """Pointers to dx and dy, scalars or per-row arrays, as one float64 per row of the array in hand."""
        dxc, dyc = _f64(dx, self.rows), _f64(dy, self.rows)
        self.keep += [dxc, dyc]
        return _v(dxc), _v(dyc)

    def outlets(self, outlets):
        """(outlet_x, outlet_y, n_outlets) of (columns, rows); None: no outlets."""
        if outlets is None:
            return None, None, -1
        ox = np.ascontiguousarray(np.asarray(outlets[0], dtype=np.int32))
        oy = np.ascontiguousarray(np.asarray(outlets[1], dtype=np.int32))
        if ox.shape != oy.shape or ox.ndim != 1:
            raise ValueError("outlets: need two equal-length 1-D index arrays (columns, rows)")
        self.keep += [ox, oy]
        return _v(ox), _v(oy), int(ox.size)

    def call(self, symbol, *args):
        """symbol[_dev | _strip](ctx, [comm,] args..., &stats) -> the stats dict.  `args`: the header's arguments between the context and
        the stats, in its order.  Device rasters: torch's work on them is waited for first."""
        if self.dev:
            import torch

            torch.cuda.synchronize(self.ctx.device)
        fn = getattr(self.ctx._lib, symbol + ("_strip" if self.strip else "_dev" if self.dev else ""))
        head = (self.ctx._h, self.comm) if self.strip else (self.ctx._h,)
        st = TdxStats()
        check(fn(*head, *args, C.byref(st)), self.ctx._h)
        return st.as_dict()


def _ret(res, stats):
    """What a Context method returns of a body's (outputs..., stats dict): all of it with stats=True, else the outputs, a single one bare."""
    return res if stats else res[0] if len(res) == 2 else res[:-1]


class _DropAnalysisStage:
    """Context.dropanalysis.  Unlike the raster stages it returns per-threshold arrays, a table text and an optimum, on the host for either side; its
    entry points are those of include/taudem_amd_dropan.h."""

    def dropanalysis(self, ad8, p, fel, ssa, outlets, *, thresh_min=5.0, thresh_max=500.0, nthresh=10, steptype=0, dx=1.0, dy=1.0, nodata=int(P_NODATA),
                     ssa_nodata=float(AREA_NODATA), grids=None, stats=False):
        """thresh, n1, n2, sums, length, total_area, table, optimum = dropanalysis(ad8, p, fel, ssa, outlets)  (src/DropAnalysis.cpp:172).

        For each of nthresh thresholds between thresh_min and thresh_max (steptype 0: log steps, else arithmetic) the stream mask ssa >= thresh is
        ordered and the elevation drops of its streams are collected: thresh float32, n1 / n2 int64 (first-order / higher-order drops), sums
        float64 [nthresh][4] (sum and sum of squares of the first-order, then of the higher-order drops), length float64 - numpy arrays on the
        host; total_area float32; table: the text of the reference's table file; optimum: the first threshold whose |t| < 2, None when there is
        none.  ssa: any float32 raster that increases downstream (ad8 itself serves); outlets: (columns, rows).  The fp64 sums are taken in a
        fixed order: the same input gives the same bits.  grids=k (a test hook) also returns, after the optimum, the order (int16, nodata -32768)
        and the start elevation carried down the stream (float32, nodata -FLT_MAX) of every cell for threshold number k."""
        return _ret(_dropanalysis(_Call(self), ad8, p, fel, ssa, outlets, thresh_min, thresh_max, nthresh, steptype, dx, dy, nodata, ssa_nodata, grids), stats)


class _PeukerDouglasStage:
    """Context.peukerdouglas; its entry points are those of include/taudem_amd_peuker.h."""

    def peukerdouglas(self, fel, nodata=float(FEL_NODATA), weights=(0.4, 0.1, 0.05), float_weights=False, out=None, stats=False):
        """ss = peukerdouglas(fel)  (src/PeukerDouglas.cpp:54): int16, 1 on the stream-source cells of the curvature-based stream definition, 0 elsewhere.

        fel is smoothed with weights = (centre, side, diagonal), the reference's -par, and every 2x2 group of the smoothed grid unflags its highest
        cell (and ties, and all four next to nodata): what stays flagged are the upward-curved cells.  float_weights=True also returns w, the same
        0 / 1 values as float32, which is what aread8(weights=w) takes: ss, w = peukerdouglas(fel, float_weights=True).  out: ss, or (ss, w)."""
        return _ret(_peukerdouglas(_Call(self), fel, nodata, weights, float_weights, out), stats)


class _StreamNetStage:
    """Context.streamnet; its entry points are those of include/taudem_amd_streamnet.h."""

    def streamnet(self, p, src, fel, ad8, outlets=None, single_watershed=False, *, dx=1.0, dy=1.0, geotransform=None, nodata=int(P_NODATA),
                  src_nodata=int(P_NODATA), out=None, phases=False, stats=False, net=None, geographic=False, links="host"):
        """ord, w, tree, coord = streamnet(p, src, fel, ad8)  (src/streamnet.cpp:372): the stream network of the stream raster src on the D8 directions p.
        net=path also writes the stream network line layer (the reference's -net: a shapefile or GeoJSON by the extension, 17 fields per link) from the
        links once the call has returned them; geographic: the raster's flag, which decides how the layer's lengths are measured.

        ord int16: the Strahler order on the stream cells (src not nodata, src > 0, p not nodata), 0 elsewhere.  w int32: the id of the link that
        drains each cell, the catchment grid catchhydrogeo and inundepth take; -2147483647 where no stream is reached; single_watershed (-sw): 1
        instead of the ids.  tree int64 (links, 9): link, first and last row of its points in coord, downstream link, the two upstream links,
        order, outlet id, magnitude.  coord float64 (points, 5): x, y, distance to the outlet along the stream, elevation, contributing area
        (ad8 times the middle row's cell area) - the rows of the reference's -tree and -coord files on one rank, in its order.
        src int32, fel / ad8 float32 (read without a nodata test).  outlets: (columns, rows[, ids]) in file order: an outlet on a stream cell ends a
        link there.  geotransform: GDAL's six numbers of the raster file (default: left edge 0, top edge 0, cells of dx x dy of the middle row).
        tree and coord are numpy arrays on the host for either side; phases=True also returns, after coord, the wall milliseconds of the call's
        phases as a dict (setup, length, compact, links, scatter, label, total).  out: (ord, w).
        links: "host" (the default) builds the links in a walk on one host core; "device" builds them on the GPU (tdx_streamnet_gpu_links: the same
        bytes; the stream cells' columns, labels and orders never leave the device).  With phases=True the dict of a device build also holds
        "links_device": the builder's sub-phases in milliseconds (classify, jump, level, number, links, rows, download), jump_rounds, level_rounds and
        workspace_bytes."""
        return _ret(_streamnet(_Call(self), p, src, fel, ad8, outlets, single_watershed, dx, dy, geotransform, nodata, src_nodata, out, phases, net, geographic, links),
                    stats)


class _OutletToolsStage:
    """Context.moveoutletstostrm and Context.connectdown; their entry points are those of include/taudem_amd_outlets.h.  Both return numpy arrays on
    the host for either side."""

    def moveoutletstostrm(self, p, src, outlets, maxdist=50, *, nodata=int(P_NODATA), src_nodata=int(P_NODATA), stats=False):
        """columns, rows, dist_moved = moveoutletstostrm(p, src, outlets)  (src/MoveOutletsToStrm.cpp:80): every outlet walks down the D8 directions p
        until it stands on a stream cell (src int32, not nodata and >= 1).

        outlets: (columns, rows).  dist_moved int32: the steps walked, 0 for an outlet that was on the stream, -1 for one that could not be moved: off
        the raster, a p outside 1..8 off the stream, a receiver off the raster, or maxdist steps without a stream cell.  columns / rows int32: the cell
        reached (with -1: the cell where the outlet gave up; the tool writes its original coordinates then)."""
        return _ret(_moveoutlets(_Call(self), p, src, outlets, maxdist, nodata, src_nodata), stats)

    def connectdown(self, p, w, ad8, movedist=10, *, nodata=int(P_NODATA), w_nodata=-2147483647, phases=False, stats=False):
        """ids, columns, rows, ad8max, moved_columns, moved_rows, id_down = connectdown(p, w, ad8)  (src/ConnectDown.cpp:79): for every watershed id of w
        (int32, any value that is not nodata, 0 .. CONNECTDOWN_MAX_ID), in ascending order, the cell of greatest ad8 (float32; the first one in
        row-major order among equals), and the cell movedist steps down p from it, with the w found there.

        All int32 but ad8max (float32).  phases=True also returns, after id_down, the device milliseconds of the phases as a dict (maxid, argmax,
        decode, walk)."""
        return _ret(_connectdown(_Call(self), p, w, ad8, movedist, nodata, w_nodata, phases), stats)


class _SinmapStage:
    """Context.sinmapsi; its entry points are those of include/taudem_amd_sinmap.h."""

    def sinmapsi(self, slp, sca, cal, regions, rminter, rmaxter, g=9.81, rhow=1000.0, scamin=None, scamax=None, *, slp_nodata=float(SLOPE_NODATA),
                 cal_nodata=-32768, out=None, stats=False):
        """si, sat = sinmapsi(slp, sca, cal, regions, rminter, rmaxter, g, rhow)  (src/SinmapSI.cpp:138): the SINMAP stability index and the saturation
        raster, float32, nodata -1.

        slp: tan of the slope angle (dinfflowdir's), sca: specific catchment area (areadinf's), cal: int16 region ids.  regions: the table of
        read_calpar() - a dict of the columns id, tmin, tmax, cmin, cmax, phimin, phimax, rhos -, a sequence of such 8-tuples, or the path of a
        -calpar file.  rminter / rmaxter: the recharge bounds, g and rhow the reference's -par; all four are rounded to float32 first, as the
        reference scans them.  scamin / scamax: the road contributions, each optional.  out: (si, sat)."""
        return _ret(_sinmapsi(_Call(self), slp, sca, cal, regions, rminter, rmaxter, g, rhow, scamin, scamax, slp_nodata, cal_nodata, out), stats)


class _TerrainIndexStage:
    """Context.terrain_indices, twi, slopearea, slopearearatio, lengtharea and setregion; their entry points are those of include/taudem_amd_indices.h."""

    def terrain_indices(self, slp, sca, m=2.0, n=1.0, want=_lib.TERRAIN_OUTPUTS, *, slp_nodata=float(SLOPE_NODATA), sca_nodata=float(AREA_NODATA), out=None,
                        stats=False):
        """twi, sa, sar = terrain_indices(slp, sca): the outputs named in `want` (any non-empty subset of "twi", "sa", "sar", returned in that order) from
        one pass over slp and sca, float32, nodata -1.

        twi = ln(sca / slp) where both have data and are > 0 (src/TWI.cpp:49); sa = slp^m * sca^n where both are >= 0, without a nodata test
        (src/SlopeArea.cpp:52); sar = slp / sca where sca has data (src/SlopeAreaRatio.cpp:49).  m and n are rounded to float32 first, as the reference
        scans them.  ln and the powers are the correctly rounded float32 (include/taudem_amd_indices.h).  out: one raster per name in `want`."""
        return _ret(_terrain_indices(_Call(self), slp, sca, m, n, want, slp_nodata, sca_nodata, out), stats)

    def twi(self, slp, sca, *, slp_nodata=float(SLOPE_NODATA), sca_nodata=float(AREA_NODATA), out=None, stats=False):
        """twi = terrain_indices(slp, sca, want=("twi",))  (src/TWI.cpp:49)."""
        return _ret(_terrain_indices(_Call(self), slp, sca, 0.0, 0.0, ("twi",), slp_nodata, sca_nodata, None if out is None else (out,)), stats)

    def slopearea(self, slp, sca, m=2.0, n=1.0, *, out=None, stats=False):
        """sa = terrain_indices(slp, sca, m, n, want=("sa",))  (src/SlopeArea.cpp:52)."""
        return _ret(_terrain_indices(_Call(self), slp, sca, m, n, ("sa",), float(SLOPE_NODATA), float(AREA_NODATA), None if out is None else (out,)), stats)

    def slopearearatio(self, slp, sca, *, sca_nodata=float(AREA_NODATA), out=None, stats=False):
        """sar = terrain_indices(slp, sca, want=("sar",))  (src/SlopeAreaRatio.cpp:49)."""
        return _ret(_terrain_indices(_Call(self), slp, sca, 0.0, 0.0, ("sar",), float(SLOPE_NODATA), sca_nodata, None if out is None else (out,)), stats)

    def lengtharea(self, plen, ad8, M=0.03, y=1.3, *, out=None, stats=False):
        """ss = lengtharea(plen, ad8)  (src/LengthArea.cpp:51): int16, 1 where ad8 >= M * plen^y, 0 where not, -32768 where plen is negative or NaN.

        plen float32 (gridnet's), ad8 float32 as aread8 leaves it: each value becomes the int32 the reference's read of the file gives (halves away
        from zero) and is compared as a float.  M and y are rounded to float32 first."""
        return _ret(_lengtharea(_Call(self), plen, ad8, M, y, out), stats)

    def setregion(self, p, gw, region_id=1, *, nodata=int(P_NODATA), gw_nodata=-2147483647, out=None, stats=False):
        """region = setregion(p, gw, region_id)  (src/SetRegion.cpp:78): int32, region_id on every cell that has data in gw (int32) or in p (int16) or
        that a neighbour's p drains into, -2147483647 on the rest."""
        return _ret(_setregion(_Call(self), p, gw, region_id, nodata, gw_nodata, out), stats)


class _EditRasterStage:
    """Context.editraster; its entry points are those of include/taudem_amd_editraster.h."""

    def editraster(self, raster, cols, rows, vals, out=None, *, nodata=int(P_NODATA), stats=False):
        """new = editraster(raster, cols, rows, vals)  (src/EditRaster.cpp:69): the int16 raster with its nodata cells as -32768 and cell (rows[k], cols[k])
        set to vals[k] for every k; a change off the raster is skipped, the last change of a cell holds, a value no int16 holds raises TdxError.

        out=raster edits a tensor (or a numpy array) in place."""
        return _ret(_editraster(_Call(self), raster, cols, rows, vals, nodata, out), stats)


class _PolygonizeStage:
    """Context.polygonize; its entry points are those of include/taudem_amd_polygonize.h."""

    def polygonize(self, w, nodata=-2147483647, *, stats=False):
        """polygons = polygonize(w): the watershed polygons of the id grid w (int32; every value that is not nodata is an id), what the toolbox step
        "Watershed Grid To Shapefile" makes of the w grid of streamnet or gagewatershed.  The boundary edges come off the device (a tensor is read where
        it is), the rings are closed on the host.  Returns a Polygons object: numpy arrays and write(path, geotransform); it owns a handle of the
        library, so use it as a context manager or close() it."""
        return _ret(_polygonize(_Call(self), w, nodata), stats)

    def polygonize_rings(self, w, nodata=-2147483647, *, rings="host", stats=False):
        """polygons = polygonize_rings(w, rings="device"): polygonize(w) with the choice of where the rings are closed.  "host": what polygonize does.
        "device": the edge columns stay on the device, the rings are closed, classified and ordered there and only the finished layer comes down; the
        arrays are the same, Polygons.ring_phases holds the ring builder's sub-phases.  Any other word raises ValueError."""
        return _ret(_polygonize(_Call(self), w, nodata, rings), stats)


class _RegionGridStage:
    """Context.regiongrid; its entry points are those of include/taudem_amd_regions.h."""

    def regiongrid(self, shape, gt, polygons=None, values=None, source=None, source_gt=None, source_nodata=-2147483647, out=None, *, workspace_words=0,
                   stats=False):
        """grid, ids = regiongrid((ny, nx), gt): the SINMAP parameter region grid on the DEM's grid (pyfiles/SIRegionTool.py), int16 with nodata 0, and
        the sorted values that occur in it.  polygons (with values, one in 1 .. 32767 per feature): a list of features, each a list of rings, each an
        (n, 2) array of x, y; a cell takes the value of the last feature whose rings hold its centre by the even-odd rule.  source (int32, with
        source_gt and source_nodata): an existing region grid, resampled by nearest neighbour without reprojection.  Neither: one region, 1 everywhere.
        gt / source_gt: GDAL's six numbers, unrotated.  The grid is a numpy array, or a tensor on this device if out= or source is one.
        workspace_words bounds the parity bitmap words of a batch of features (0: the library's default).  stats=True also asks for the phase times
        (stats["phases"]), which drains the stream at the end of every phase of every batch; without it nothing is drained between the kernels."""
        return _ret(_regiongrid(_Call(self), shape, gt, polygons, values, source, source_gt, source_nodata, out, workspace_words, phases=stats), stats)


class Context(_DropAnalysisStage, _PeukerDouglasStage, _StreamNetStage, _OutletToolsStage, _SinmapStage, _TerrainIndexStage, _EditRasterStage, _PolygonizeStage,
              _RegionGridStage):
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

    # ---- stages: thin signatures over the shared bodies below (_pitremove(...) etc.), on a _Call frame of this context ---------------
    def pitremove(self, dem, nodata=-9999.0, mask=None, fourway=False, out=None, stats=False):
        """fel = flood(dem)  (src/flood.cpp:50)."""
        return _ret(_pitremove(_Call(self), dem, nodata, mask, fourway, out), stats)

    def d8flowdir(self, fel, nodata=float(FEL_NODATA), dx=1.0, dy=1.0, want_slope=True, out=None, stats=False):
        """p, sd8 = setdird8(fel)  (src/d8.cpp:181).  dx, dy: scalars or per-row arrays (metres)."""
        return _ret(_d8flowdir(_Call(self), fel, nodata, dx, dy, want_slope, out), stats)

    def aread8(self, p, nodata=int(P_NODATA), weights=None, weights_nodata=-9999.0, contcheck=True, outlets=None, out=None, stats=False):
        """ad8 = aread8(p)  (src/aread8.cpp:56).  outlets: (columns, rows) global indices or None."""
        return _ret(_aread8(_Call(self), p, nodata, weights, weights_nodata, contcheck, outlets, out), stats)

    def d8flowpathextremeup(self, p, sa, nodata=int(P_NODATA), usemax=True, contcheck=True, outlets=None, out=None, stats=False):
        """ssa = d8flowpathextremeup(p, sa)  (src/D8flowpathextremeup.cpp:58): upstream max / min of sa along D8 flow paths (nodata -FLT_MAX)."""
        return _ret(_d8flowpathextremeup(_Call(self), p, sa, nodata, usemax, contcheck, outlets, out), stats)

    def gridnet(self, p, nodata=int(P_NODATA), dx=1.0, dy=1.0, mask=None, thresh=0, outlets=None, stats=False):
        """plen, tlen, gord = gridnet(p)  (src/gridnet.cpp:54).  mask: int32 raster, cells with mask >= thresh are evaluated;
        outlets: (columns, rows) - only their upstream closure is evaluated."""
        return _ret(_gridnet(_Call(self), p, nodata, dx, dy, mask, thresh, outlets), stats)

    def threshold(self, ssa, thresh, nodata=-1.0, mask=None, stats=False):
        """src = threshold(ssa)  (src/Threshold.cpp:49): 1 where ssa >= thresh (and mask >= 0), 0 elsewhere, -32768 where ssa is nodata."""
        f = _Call(self)
        pa = f.raster(ssa, np.float32, "ssa")
        pm = f.raster(mask, np.float32, "mask")
        src, ps = f.out(None, np.int16, "src")
        return _ret((src, f.call("tdx_threshold", pa, f.nx, f.ny, float(nodata), pm, float(thresh), ps)), stats)

    def dinfflowdir(self, fel, nodata=float(FEL_NODATA), dx=1.0, dy=1.0, out=None, stats=False):
        """ang, slp = setdir(fel)  (src/dinf.cpp:109)."""
        return _ret(_dinfflowdir(_Call(self), fel, nodata, dx, dy, out), stats)

    def areadinf(self, ang, nodata=float(ANG_NODATA), dx=1.0, dy=1.0, weights=None, contcheck=True, outlets=None, out=None, stats=False):
        """sca = area(ang)  (src/areadinf.cpp:53)."""
        return _ret(_areadinf(_Call(self), ang, nodata, dx, dy, weights, contcheck, outlets, out), stats)

    def dinfdecayaccum(self, ang, dm, nodata=float(ANG_NODATA), dm_nodata=-9999.0, dx=1.0, dy=1.0, weights=None, contcheck=True,
                       outlets=None, out=None, stats=False):
        """dsca = dmarea(ang, dm)  (src/dinfdecayaccum.cpp:61)."""
        return _ret(_dinfdecayaccum(_Call(self), ang, dm, nodata, dm_nodata, dx, dy, weights, contcheck, outlets, out), stats)

    def dinfupdependence(self, ang, dg, nodata=float(ANG_NODATA), dx=1.0, dy=1.0, stats=False):
        """dep = depgrd(ang, dg)  (src/DinfUpDependence.cpp:52): dg int32, dep float32 (nodata -1)."""
        return _ret(_dinfupdependence(_Call(self), ang, dg, nodata, dx, dy), stats)

    def dinfrevaccum(self, ang, w, nodata=float(ANG_NODATA), w_nodata=-9999.0, dx=1.0, dy=1.0, stats=False):
        """racc, dmax = dsaccum(ang, w)  (src/DinfRevAccum.cpp:51): float32, nodata -FLT_MAX."""
        return _ret(_dinfrevaccum(_Call(self), ang, w, nodata, w_nodata, dx, dy), stats)

    def dinfdistdown(self, ang, src, fel=None, *, stat="ave", kind="v", weights=None, weights_nodata=-9999.0, contcheck=True, dx=1.0, dy=1.0,
                     nodata=float(ANG_NODATA), fel_nodata=float(FEL_NODATA), stats=False):
        """dd = dinfdistdown(ang, fel, src, w)  (src/DinfDistDown.cpp:66): distance from each cell down to the stream (src int16 >= 1).

        kind "h" horizontal, "v" vertical drop (with stat "ave": HAND), "p" Pythagorean, "s" surface; stat "ave", "max" or "min" over
        the receivers.  `fel` is required for v, p and s; `weights` scale the horizontal steps of h, p and s (v ignores them, as the
        reference does).  dd float32, nodata -FLT_MAX."""
        return _ret(_dinfdistdown(_Call(self), ang, src, fel, stat, kind, weights, weights_nodata, contcheck, dx, dy, nodata, fel_nodata), stats)

    def d8hdisttostrm(self, p, src, thresh=1, *, dx=1.0, dy=1.0, nodata=int(P_NODATA), src_nodata=-2147483647, stats=False):
        """dist = distgrid(p, src)  (src/D8HDistToStrm.cpp:57): horizontal distance along the D8 flow path down to the stream.

        Stream cells are those where src (int32, the reference's LONG read) is not src_nodata and is >= thresh, whatever p is there;
        they get 0.  dist float32, nodata -FLT_MAX (off the raster, into a cell without a result, around a cycle)."""
        return _ret(_d8hdisttostrm(_Call(self), p, src, thresh, dx, dy, nodata, src_nodata), stats)

    def d8vdisttostrm(self, p, fel, src, thresh=1, *, nodata=int(P_NODATA), src_nodata=-2147483647, stats=False):
        """dist = d8vdistdown(p, fel, src)  (src/D8VDistToStrm.cpp:58): vertical drop along the D8 flow path down to the stream.

        Stream cells as for d8hdisttostrm; every other cell gets (fel - fel(receiver)) + dist(receiver) in float32.  fel is read with no
        nodata test, as in the reference.  dist float32, nodata -FLT_MAX."""
        return _ret(_d8vdisttostrm(_Call(self), p, fel, src, thresh, nodata, src_nodata), stats)

    def flowdircond(self, p, z, *, nodata=int(P_NODATA), z_nodata=float(FEL_NODATA), stats=False):
        """zfdc = flowdircond(p, z)  (src/flowdircond.cpp:54): z conditioned along the D8 directions - from the ridges downstream every
        cell becomes the minimum of its own z and the conditioned z of the cells that drain into it.

        Cells the reference's queue never reaches (no valid direction, below a p == 0 cell, on or below a cycle) and cells with nodata z
        keep their input value; the result carries z's nodata value."""
        return _ret(_flowdircond(_Call(self), p, z, nodata, z_nodata), stats)

    def slopeavedown(self, p, fel, dn=50.0, *, dx=1.0, dy=1.0, niter=None, nodata=int(P_NODATA), fel_nodata=float(FEL_NODATA), stats=False):
        """slpd = sloped(p, fel, dn)  (src/SlopeAveDown.cpp:59): the slope from each cell to the cell the distance dn down its D8 flow path.

        niter (default int(dn / min(dx, dy) of the middle row) + 1, the reference's count; not capped) synchronous one-step pulls along
        the D8 pointer.  dn must be finite and not negative.  slpd float32, nodata -FLT_MAX."""
        return _ret(_slopeavedown(_Call(self), p, fel, dn, int(niter) if niter else 0, dx, dy, nodata, fel_nodata), stats)   # 0: the library counts

    def catchhydrogeo(self, hand, catch, slp, ids, stages, *, dx=1.0, dy=1.0, hand_nodata=float(ANG_NODATA), catch_nodata=-9999, slp_nodata=-1.0, stats=False):
        """count, surface, bed, volume, catcharea = catchhydrogeo(hand, catch, slp, ids, stages)  (src/CatchHydroGeo.cpp:69).

        Per listed catchment id and stage: the cells of the catchment whose hand is below the stage (or within 1e-6 of 0), their plan area,
        bed area and volume; and each catchment's whole plan area.  ids: int32 list (the last row of a repeated id wins, earlier rows stay 0);
        stages: float64, any order.  count int32 and surface / bed / volume float64 are [len(stages)][len(ids)], catcharea float64 [len(ids)];
        all numpy arrays on the host.  The fp64 sums are taken in a fixed order: the same input gives the same bits."""
        f = _Call(self)
        ph = f.raster(hand, np.float32, "hand")
        pc = f.raster(catch, np.int32, "catch")
        ps = f.raster(slp, np.float32, "slp")
        pdx, pdy = f.cells(dx, dy)
        ids, stages = _flat(ids, np.int32), _flat(stages, np.float64)
        nc, nh = ids.size, stages.size
        count = np.zeros((nh, nc), np.int32)
        surface, bed, volume = (np.zeros((nh, nc), np.float64) for _ in range(3))
        catcharea = np.zeros(nc, np.float64)
        st = f.call("tdx_catchhydrogeo", ph, pc, ps, f.nx, f.ny, float(hand_nodata), int(catch_nodata), float(slp_nodata), pdx, pdy, _v(ids), nc, _v(stages), nh,
                    _v(count), _v(surface), _v(bed), _v(volume), _v(catcharea))
        return _ret((count, surface, bed, volume, catcharea, st), stats)

    def inundepth(self, hand, catch, ids, depth, *, mask=None, area=True, dx=1.0, dy=1.0, hand_nodata=float(ANG_NODATA), catch_nodata=-9999, mask_nodata=-32768,
                  stats=False):
        """map, area = inundepth(hand, catch, ids, depth)  (src/InunDepth.cpp:53, the raster part).

        ids / depth: one forecast depth (float32) per id, the last row of a repeated id wins.  map float32, nodata -3.0e38: depth - hand where
        catch and hand have data, depth >= 0 and depth > hand + 0.001.  mask (int16): as in the reference, with a mask every cell of the map is
        nodata.  area (float32 per row, None with area=False): plan area of the cells with depth > 0 and depth - hand > 0, at the winning row
        of each id, 0 elsewhere; summed in fp64 and rounded once."""
        ids, depth = _flat(ids, np.int32), _flat(depth, np.float32)
        if ids.size != depth.size:
            raise ValueError("ids and depth: need equal lengths")
        f = _Call(self)
        ph = f.raster(hand, np.float32, "hand")
        pc = f.raster(catch, np.int32, "catch")
        pm = f.raster(mask, np.int16, "mask")
        pdx, pdy = f.cells(dx, dy)
        out, po = f.out(None, np.float32, "map")
        wet = np.zeros(ids.size, np.float32) if area else None
        st = f.call("tdx_inundepth", ph, pc, pm, f.nx, f.ny, float(hand_nodata), int(catch_nodata), int(mask_nodata), pdx, pdy, _v(ids), _v(depth), ids.size, po,
                    _v(wet) if area else None)
        return _ret((out, wet, st), stats)

    def gagewatershed(self, p, outlets, *, nodata=int(P_NODATA), stats=False):
        """gw, id_table = gagewatershed(p, outlets)  (src/gagewatershed.cpp:56): every cell gets the id of the first gauge downstream of it.

        outlets: (columns, rows[, ids]) global indices (ids default to 1..n, as the outlet reader's); outlets off the raster are skipped and
        the first one on a cell wins.  gw int32, nodata -2147483647.  id_table: int32 array (k, 2) of the `-id` file's lines (id, iddown)
        for the k placed outlets in input order; iddown is -1 where the gauge's downstream neighbour is off the raster or unlabelled."""
        ids = outlets[2] if len(outlets) > 2 else np.arange(1, np.size(outlets[0]) + 1, dtype=np.int32)
        return _ret(_gagewatershed(_Call(self), p, outlets[0], outlets[1], ids, nodata), stats)

    def dinfdistup(self, ang, fel=None, *, stat="ave", kind="h", weights=None, weights_nodata=-9999.0, contcheck=True, thresh=0.0, dx=1.0, dy=1.0,
                   nodata=float(ANG_NODATA), fel_nodata=float(FEL_NODATA), stats=False):
        """du = dinfdistup(ang, fel, w)  (src/DinfDistUp.cpp:65): distance from each cell up to the ridge over the neighbours that drain into it.

        kind "h" horizontal, "v" vertical rise, "p" Pythagorean, "s" surface; stat "ave", "max" or "min" over the contributors; a
        neighbour contributes only if its proportion exceeds `thresh`.  `fel` is required for v, p and s; `weights` scale the horizontal
        steps of h, p and s (v ignores them, as the reference does).  du float32, nodata -FLT_MAX; ridge cells get 0."""
        return _ret(_dinfdistup(_Call(self), ang, fel, stat, kind, weights, weights_nodata, contcheck, thresh, dx, dy, nodata, fel_nodata), stats)

    def retlimflow(self, ang, wg, rc, *, dx=1.0, dy=1.0, nodata=float(ANG_NODATA), wg_nodata=-9999.0, rc_nodata=-9999.0, stats=False):
        """qrl = retlimro(ang, wg, rc)  (src/RetlimFlow.cpp:53): retention limited runoff, max(0, inflow + wg - rc) accumulated along the
        D-infinity flow.  A cell whose wg or rc is nodata has no value, and neither has anything downstream of it.  qrl float32, nodata -FLT_MAX."""
        return _ret(_retlimflow(_Call(self), ang, wg, rc, dx, dy, nodata, wg_nodata, rc_nodata), stats)

    def dinfavalanche(self, ang, fel, ass, *, thresh=0.2, alpha=18.0, direct=False, dx=1.0, dy=1.0, geo=None, geographic=False, nodata=float(ANG_NODATA),
                      fel_nodata=float(FEL_NODATA), ass_nodata=-32768, stats=False):
        """rz, dfs = avalancherunoutgrd(ang, fel, ass)  (src/DinfAvalanche.cpp:62): the runout zone below the source cells (ass > 0, int16) as the
        angle to the source in degrees, and the distance from the source - along the flow path, or with direct=True as a straight line in
        the raster's coordinates: geo = (xleftedge, ytopedge, dlon, dlat), by default (0, ny * dy[0], dx[0], dy[0]); needed when
        geographic, where dlon / dlat are degrees.  float32, nodata -FLT_MAX."""
        return _ret(_dinfavalanche(_Call(self), ang, fel, ass, thresh, alpha, direct, dx, dy, geo, geographic, nodata, fel_nodata, ass_nodata), stats)

    def dinfconclimaccum(self, ang, dm, dg, q, csol=1.0, nodata=float(ANG_NODATA), dm_nodata=-9999.0, q_nodata=-9999.0, dx=1.0, dy=1.0, contcheck=True,
                         outlets=None, stats=False):
        """ctpt = dsllArea(ang, dm, dg, q)  (src/DinfConcLimAccum.cpp:61): dg int16, ctpt float32 (nodata -FLT_MAX)."""
        return _ret(_dinfconclimaccum(_Call(self), ang, dm, dg, q, csol, nodata, dm_nodata, q_nodata, dx, dy, contcheck, outlets), stats)

    def dinftranslimaccum(self, ang, tsup, tc, cs=None, nodata=float(ANG_NODATA), tsup_nodata=-9999.0, tc_nodata=-9999.0, cs_nodata=-9999.0, dx=1.0, dy=1.0,
                          contcheck=True, outlets=None, stats=False):
        """tla, tdep, ctpt = tlaccum(ang, tsup, tc[, cs])  (src/DinfTransLimAccum.cpp:61): float32, nodata -FLT_MAX; ctpt is None without cs."""
        return _ret(_dinftranslimaccum(_Call(self), ang, tsup, tc, cs, nodata, tsup_nodata, tc_nodata, cs_nodata, dx, dy, contcheck, outlets), stats)

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


# ---- the tools: one marshalling body each, for Context.<tool> and StripPipeline.<tool> --------------------------------------------------
# f is the _Call frame of either; every body returns (outputs..., stats dict).  The arguments of f.call are the header's, in its order.
def _pitremove(f, dem, nodata, mask, fourway, out):
    pz = f.raster(dem, np.float32, "dem")
    pm = f.raster(mask, np.int16, "mask")
    fel, pf = f.out(out, np.float32, "fel")
    return fel, f.call("tdx_pitremove", pz, f.nx, f.ny, float(nodata), pm, int(bool(fourway)), pf)


def _d8flowdir(f, fel, nodata, dx, dy, want_slope, out):
    pz = f.raster(fel, np.float32, "fel")
    pdx, pdy = f.cells(dx, dy)
    p, pp = f.out(out[0] if out is not None else None, np.int16, "p")
    sd8, ps = f.out(out[1] if out is not None else None, np.float32, "sd8") if want_slope else (None, None)
    return p, sd8, f.call("tdx_d8flowdir", pz, f.nx, f.ny, float(nodata), pdx, pdy, pp, ps)


def _aread8(f, p, nodata, weights, weights_nodata, contcheck, outlets, out):
    pp = f.raster(p, np.int16, "p")
    pw = f.raster(weights, np.float32, "weights")
    ad8, pa = f.out(out, np.float32, "ad8")
    ox, oy, no = f.outlets(outlets)
    return ad8, f.call("tdx_aread8", pp, f.nx, f.ny, int(nodata), pw, float(weights_nodata), int(bool(contcheck)), ox, oy, no, pa)


def _d8flowpathextremeup(f, p, sa, nodata, usemax, contcheck, outlets, out):
    pp = f.raster(p, np.int16, "p")
    pa = f.raster(sa, np.float32, "sa")
    ssa, ps = f.out(out, np.float32, "ssa")
    ox, oy, no = f.outlets(outlets)
    return ssa, f.call("tdx_d8flowpathextremeup", pp, f.nx, f.ny, int(nodata), pa, int(bool(usemax)), int(bool(contcheck)), ox, oy, no, ps)


def _gridnet(f, p, nodata, dx, dy, mask, thresh, outlets):
    pp = f.raster(p, np.int16, "p")
    pm = f.raster(mask, np.int32, "mask")
    pdx, pdy = f.cells(dx, dy)
    plen, ppl = f.out(None, np.float32, "plen")
    tlen, ptl = f.out(None, np.float32, "tlen")
    gord, pgo = f.out(None, np.int16, "gord")
    ox, oy, no = f.outlets(outlets)
    return plen, tlen, gord, f.call("tdx_gridnet", pp, f.nx, f.ny, int(nodata), pdx, pdy, pm, int(thresh), ox, oy, no, ppl, ptl, pgo)


def _dinfflowdir(f, fel, nodata, dx, dy, out):
    pz = f.raster(fel, np.float32, "fel")
    pdx, pdy = f.cells(dx, dy)
    ang, pa = f.out(out[0] if out is not None else None, np.float32, "ang")
    slp, ps = f.out(out[1] if out is not None else None, np.float32, "slp")
    return ang, slp, f.call("tdx_dinfflowdir", pz, f.nx, f.ny, float(nodata), pdx, pdy, pa, ps)


def _areadinf(f, ang, nodata, dx, dy, weights, contcheck, outlets, out):
    pa = f.raster(ang, np.float32, "ang")
    pw = f.raster(weights, np.float32, "weights")
    pdx, pdy = f.cells(dx, dy)
    sca, ps = f.out(out, np.float32, "sca")
    ox, oy, no = f.outlets(outlets)
    return sca, f.call("tdx_areadinf", pa, f.nx, f.ny, float(nodata), pdx, pdy, pw, int(bool(contcheck)), ox, oy, no, ps)


def _dinfdecayaccum(f, ang, dm, nodata, dm_nodata, dx, dy, weights, contcheck, outlets, out):
    pa = f.raster(ang, np.float32, "ang")
    pd = f.raster(dm, np.float32, "dm")
    pw = f.raster(weights, np.float32, "weights")
    pdx, pdy = f.cells(dx, dy)
    dsca, ps = f.out(out, np.float32, "dsca")
    ox, oy, no = f.outlets(outlets)
    return dsca, f.call("tdx_dinfdecayaccum", pa, f.nx, f.ny, float(nodata), pdx, pdy, pd, float(dm_nodata), pw, int(bool(contcheck)), ox, oy, no, ps)


def _dinfupdependence(f, ang, dg, nodata, dx, dy):
    pa = f.raster(ang, np.float32, "ang")
    pg = f.raster(dg, np.int32, "dg")
    pdx, pdy = f.cells(dx, dy)
    dep, po = f.out(None, np.float32, "dep")
    return dep, f.call("tdx_dinfupdependence", pa, f.nx, f.ny, float(nodata), pdx, pdy, pg, po)


def _dinfrevaccum(f, ang, w, nodata, w_nodata, dx, dy):
    pa = f.raster(ang, np.float32, "ang")
    pw = f.raster(w, np.float32, "w")
    pdx, pdy = f.cells(dx, dy)
    racc, pr = f.out(None, np.float32, "racc")
    dmax, pm = f.out(None, np.float32, "dmax")
    return racc, dmax, f.call("tdx_dinfrevaccum", pa, f.nx, f.ny, float(nodata), pdx, pdy, pw, float(w_nodata), pr, pm)


def _dinfdistdown(f, ang, src, fel, stat, kind, weights, weights_nodata, contcheck, dx, dy, nodata, fel_nodata):
    sm, tm, fel, weights = _distdown_mode(stat, kind, fel, weights)
    pa = f.raster(ang, np.float32, "ang")
    ps = f.raster(src, np.int16, "src")
    pf = f.raster(fel, np.float32, "fel")
    pw = f.raster(weights, np.float32, "weights")
    pdx, pdy = f.cells(dx, dy)
    dd, po = f.out(None, np.float32, "dd")
    return dd, f.call("tdx_dinfdistdown", pa, f.nx, f.ny, float(nodata), pdx, pdy, pf, float(fel_nodata), ps, pw, float(weights_nodata), sm, tm,
                      int(bool(contcheck)), po)


def _dinfdistup(f, ang, fel, stat, kind, weights, weights_nodata, contcheck, thresh, dx, dy, nodata, fel_nodata):
    sm, tm, fel, weights = _distdown_mode(stat, kind, fel, weights)
    pa = f.raster(ang, np.float32, "ang")
    pf = f.raster(fel, np.float32, "fel")
    pw = f.raster(weights, np.float32, "weights")
    pdx, pdy = f.cells(dx, dy)
    du, po = f.out(None, np.float32, "du")
    return du, f.call("tdx_dinfdistup", pa, f.nx, f.ny, float(nodata), pdx, pdy, pf, float(fel_nodata), pw, float(weights_nodata), sm, tm,
                      int(bool(contcheck)), float(thresh), po)


def _d8hdisttostrm(f, p, src, thresh, dx, dy, nodata, src_nodata):
    pp = f.raster(p, np.int16, "p")
    ps = f.raster(src, np.int32, "src")
    pdx, pdy = f.cells(dx, dy)
    dist, po = f.out(None, np.float32, "dist")
    return dist, f.call("tdx_d8hdisttostrm", pp, f.nx, f.ny, int(nodata), ps, int(src_nodata), int(thresh), pdx, pdy, po)


def _d8vdisttostrm(f, p, fel, src, thresh, nodata, src_nodata):
    pp = f.raster(p, np.int16, "p")
    pf = f.raster(fel, np.float32, "fel")
    ps = f.raster(src, np.int32, "src")
    dist, po = f.out(None, np.float32, "dist")
    return dist, f.call("tdx_d8vdisttostrm", pp, f.nx, f.ny, int(nodata), pf, ps, int(src_nodata), int(thresh), po)


def _flowdircond(f, p, z, nodata, z_nodata):
    pp = f.raster(p, np.int16, "p")
    pz = f.raster(z, np.float32, "z")
    zfdc, po = f.out(None, np.float32, "zfdc")
    return zfdc, f.call("tdx_flowdircond", pp, f.nx, f.ny, int(nodata), pz, float(z_nodata), po)


def _slopeavedown(f, p, fel, dn, niter, dx, dy, nodata, fel_nodata):
    pp = f.raster(p, np.int16, "p")
    pf = f.raster(fel, np.float32, "fel")
    pdx, pdy = f.cells(dx, dy)
    slpd, po = f.out(None, np.float32, "slpd")
    return slpd, f.call("tdx_slopeavedown", pp, f.nx, f.ny, int(nodata), pf, float(fel_nodata), pdx, pdy, float(dn), niter, po)


def _gagewatershed(f, p, cols, rows, ids, nodata):
    ox, oy, ids = _flat(cols, np.int32), _flat(rows, np.int32), _flat(ids, np.int32)
    if ox.shape != oy.shape or ox.shape != ids.shape:
        raise ValueError("outlets: need equal-length 1-D arrays (columns, rows[, ids])")
    pp = f.raster(p, np.int16, "p")
    gw, pg = f.out(None, np.int32, "gw")
    placed = np.zeros(ox.size + 1, np.int32)
    iddown = np.zeros(ox.size + 1, np.int32)
    st = f.call("tdx_gagewatershed", pp, f.nx, f.ny, int(nodata), _v(ox), _v(oy), _v(ids), int(ox.size), pg, _v(placed), _v(iddown))
    keep = placed[:ox.size] > 0
    return gw, np.stack([ids[keep], iddown[:ox.size][keep]], axis=1).astype(np.int32), st


def _retlimflow(f, ang, wg, rc, dx, dy, nodata, wg_nodata, rc_nodata):
    pa = f.raster(ang, np.float32, "ang")
    pw = f.raster(wg, np.float32, "wg")
    pr = f.raster(rc, np.float32, "rc")
    pdx, pdy = f.cells(dx, dy)
    qrl, po = f.out(None, np.float32, "qrl")
    return qrl, f.call("tdx_retlimflow", pa, f.nx, f.ny, float(nodata), pdx, pdy, pw, float(wg_nodata), pr, float(rc_nodata), po)


def _dinfavalanche(f, ang, fel, ass, thresh, alpha, direct, dx, dy, geo, geographic, nodata, fel_nodata, ass_nodata, whole=()):
    """whole: (row0, ny_total), where a strip lies in the whole raster - the two arguments only tdx_dinfavalanche_strip has."""
    pa = f.raster(ang, np.float32, "ang")
    pf = f.raster(fel, np.float32, "fel")
    ps = f.raster(ass, np.int16, "ass")
    pdx, pdy = f.cells(dx, dy)
    rz, pz = f.out(None, np.float32, "rz")
    dfs, pd = f.out(None, np.float32, "dfs")
    g4 = None if geo is None else np.ascontiguousarray(np.asarray(geo, dtype=np.float64).reshape(4))
    return rz, dfs, f.call("tdx_dinfavalanche", pa, f.nx, f.ny, float(nodata), pdx, pdy, pf, float(fel_nodata), ps, int(ass_nodata), float(thresh), float(alpha),
                           0 if direct else 1, None if g4 is None else _v(g4), int(bool(geographic)), *whole, pz, pd)


def _dinfconclimaccum(f, ang, dm, dg, q, csol, nodata, dm_nodata, q_nodata, dx, dy, contcheck, outlets):
    pa = f.raster(ang, np.float32, "ang")
    pm = f.raster(dm, np.float32, "dm")
    pg = f.raster(dg, np.int16, "dg")
    pq = f.raster(q, np.float32, "q")
    pdx, pdy = f.cells(dx, dy)
    ctpt, po = f.out(None, np.float32, "ctpt")
    ox, oy, no = f.outlets(outlets)
    return ctpt, f.call("tdx_dinfconclimaccum", pa, f.nx, f.ny, float(nodata), pdx, pdy, pm, float(dm_nodata), pg, pq, float(q_nodata), float(csol),
                        int(bool(contcheck)), ox, oy, no, po)


def _dinftranslimaccum(f, ang, tsup, tc, cs, nodata, tsup_nodata, tc_nodata, cs_nodata, dx, dy, contcheck, outlets):
    pa = f.raster(ang, np.float32, "ang")
    ps = f.raster(tsup, np.float32, "tsup")
    pc = f.raster(tc, np.float32, "tc")
    pi = f.raster(cs, np.float32, "cs")
    pdx, pdy = f.cells(dx, dy)
    tla, pt = f.out(None, np.float32, "tla")
    tdep, pd = f.out(None, np.float32, "tdep")
    ctpt, po = f.out(None, np.float32, "ctpt") if cs is not None else (None, None)
    ox, oy, no = f.outlets(outlets)
    return tla, tdep, ctpt, f.call("tdx_dinftranslimaccum", pa, f.nx, f.ny, float(nodata), pdx, pdy, ps, float(tsup_nodata), pc, float(tc_nodata), pi,
                                   float(cs_nodata), int(bool(contcheck)), ox, oy, no, pt, pd, po)


def _peukerdouglas(f, fel, nodata, weights, float_weights, out):
    pz = f.raster(fel, np.float32, "fel")
    if len(weights) != 3:
        raise ValueError("weights: need (centre, side, diagonal)")
    o_ss, o_w = (out if float_weights else (out, None)) if out is not None else (None, None)
    ss, ps = f.out(o_ss, np.int16, "ss")
    w, pw = f.out(o_w, np.float32, "w") if float_weights else (None, None)
    st = f.call("tdx_peukerdouglas", pz, f.nx, f.ny, float(nodata), float(weights[0]), float(weights[1]), float(weights[2]), ps, pw)
    return (ss, w, st) if float_weights else (ss, st)


def read_calpar(path):
    """The region table of a SinmapSI -calpar file (one header line, then id,tmin,tmax,cmin,cmax,phimin,phimax,rhos per region, scanned as the
    reference scans them): a dict of numpy columns, id int32 and the rest float32, in file order.  No GPU is needed.  A file that cannot be read
    raises TdxError with code 15, a data line with fewer than 8 fields one that names the line."""
    import os

    lib = _lib.load()
    n = C.c_int32(0)
    check(lib.tdx_sinmap_read_calpar(os.fsencode(path), 0, *([None] * 8), C.byref(n)))
    cols = {k: np.zeros(n.value, np.int32 if k == "id" else np.float32) for k in _lib.SINMAP_FIELDS}
    check(lib.tdx_sinmap_read_calpar(os.fsencode(path), n.value, *[_v(cols[k]) for k in _lib.SINMAP_FIELDS], C.byref(n)))
    return cols


def _regions(regions):
    """The eight columns of a region table given as read_calpar()'s dict, as rows of 8 values, or as a path."""
    import os

    if isinstance(regions, (str, bytes, os.PathLike)):
        regions = read_calpar(regions)
    if isinstance(regions, dict):
        cols = [regions[k] for k in _lib.SINMAP_FIELDS]
    else:
        rows = [tuple(r) for r in regions]
        if any(len(r) != 8 for r in rows):
            raise ValueError("regions: need (id, tmin, tmax, cmin, cmax, phimin, phimax, rhos) per region")
        cols = [[r[k] for r in rows] for k in range(8)]
    cols = [_flat(c, np.int32 if k == 0 else np.float32) for k, c in enumerate(cols)]
    if any(c.size != cols[0].size for c in cols):
        raise ValueError("regions: columns of different lengths")
    return cols


def _sinmapsi(f, slp, sca, cal, regions, rminter, rmaxter, g, rhow, scamin, scamax, slp_nodata, cal_nodata, out):
    ps = f.raster(slp, np.float32, "slp")
    pa = f.raster(sca, np.float32, "sca")
    pmin, pmax = f.raster(scamin, np.float32, "scamin"), f.raster(scamax, np.float32, "scamax")
    pc = f.raster(cal, np.int16, "cal")
    cols = _regions(regions)
    f.keep += cols
    o_si, o_sat = out if out is not None else (None, None)
    si, psi = f.out(o_si, np.float32, "si")
    sat, psat = f.out(o_sat, np.float32, "sat")
    st = f.call("tdx_sinmapsi", ps, pa, pmin, pmax, pc, f.nx, f.ny, float(slp_nodata), float(cal_nodata), int(cols[0].size), *[_v(c) for c in cols],
                float(np.float32(rminter)), float(np.float32(rmaxter)), float(g), float(rhow), psi, psat)
    return si, sat, st


def _terrain_indices(f, slp, sca, m, n, want, slp_nodata, sca_nodata, out):
    want = tuple(want)
    if not want or len(set(want)) != len(want) or any(w not in _lib.TERRAIN_OUTPUTS for w in want):
        raise ValueError(f"want: need a non-empty selection of {_lib.TERRAIN_OUTPUTS} without repeats, not {want!r}")
    given = (None,) * len(want) if out is None else tuple(out)
    if len(given) != len(want):
        raise ValueError("out: need one raster per name in want")
    ps = f.raster(slp, np.float32, "slp")
    pa = f.raster(sca, np.float32, "sca")
    res = {w: f.out(g, np.float32, w) for w, g in zip(want, given)}
    ptr = [res[w][1] if w in res else None for w in _lib.TERRAIN_OUTPUTS]
    st = f.call("tdx_terrain_indices", ps, pa, f.nx, f.ny, float(slp_nodata), float(sca_nodata), float(np.float32(m)), float(np.float32(n)), *ptr)
    return tuple(res[w][0] for w in want) + (st,)


def _lengtharea(f, plen, ad8, M, y, out):
    pl = f.raster(plen, np.float32, "plen")
    pa = f.raster(ad8, np.float32, "ad8")
    ss, ps = f.out(out, np.int16, "ss")
    return ss, f.call("tdx_lengtharea", pl, pa, f.nx, f.ny, float(np.float32(M)), float(np.float32(y)), ps)


def _setregion(f, p, gw, region_id, nodata, gw_nodata, out):
    pp = f.raster(p, np.int16, "p")
    pg = f.raster(gw, np.int32, "gw")
    o, po = f.out(out, np.int32, "region")
    return o, f.call("tdx_setregion", pp, pg, f.nx, f.ny, int(nodata), int(gw_nodata), int(region_id), po)


def _editraster(f, raster, cols, rows, vals, nodata, out, row0=None):
    """row0: a strip's first owned row in the raster (rows are then GLOBAL rows); None for a Context."""
    pi = f.raster(raster, np.int16, "raster")
    cx, cy, cv = (_flat(a, np.int64) for a in (cols, rows, vals))
    if not cx.shape == cy.shape == cv.shape:
        raise ValueError("cols, rows, vals: need three equal-length 1-D arrays")
    lim = np.iinfo(np.int32)
    # cells beyond int32 are off every raster; values beyond it are for the library to refuse: both keep that meaning after the clip
    cx, cy, cv = (np.ascontiguousarray(np.clip(a, lim.min, lim.max).astype(np.int32)) for a in (cx, cy, cv))
    f.keep += [cx, cy, cv]
    n = int(cx.size)
    o, po = f.out(out, np.int16, "out")
    where = (f.nx, f.ny) if row0 is None else (f.nx, f.ny, int(row0))
    return o, f.call("tdx_editraster", pi, *where, int(nodata), _v(cx) if n else None, _v(cy) if n else None, _v(cv) if n else None, n, po)


def read_changes(path):
    """x, y, vals (float64, float64, int32) of an EditRaster change file: the first line is skipped, then "x,y,value" records up to the first one that does
    not scan (src/EditRaster.cpp:124-133).  TdxError: the file cannot be opened, or a value is outside -32768 .. 32767.  No GPU is touched."""
    lib = _lib.load()
    n = C.c_int64(0)
    check(lib.tdx_editraster_read_changes(os.fsencode(path), 0, None, None, None, C.byref(n)))
    x, y, v = np.zeros(n.value, np.float64), np.zeros(n.value, np.float64), np.zeros(n.value, np.int32)
    if n.value:
        check(lib.tdx_editraster_read_changes(os.fsencode(path), n.value, _v(x), _v(y), _v(v), C.byref(n)))
    return x, y, v


def _dropanalysis(f, ad8, p, fel, ssa, outlets, thresh_min, thresh_max, nthresh, steptype, dx, dy, nodata, ssa_nodata, grids):
    """Context: (thresh, n1, n2, sums, length, total_area, table, optimum[, order, elevout], stats).  A strip: its own (thresh, n1, n2, sums, length,
    outlet_term[, order, elevout], stats) - outlet_term float32 per outlet, ad8 of the strip's terminal outlets and 0 elsewhere."""
    pa = f.raster(ad8, np.float32, "ad8")
    pp = f.raster(p, np.int16, "p")
    pf = f.raster(fel, np.float32, "fel")
    ps = f.raster(ssa, np.float32, "ssa")
    pdx, pdy = f.cells(dx, dy)
    if outlets is None:
        raise ValueError("outlets: dropanalysis needs the outlets (columns, rows)")
    ox, oy, no = f.outlets(outlets)
    nt = int(nthresh)
    if nt < 2:
        raise ValueError("nthresh: the number of thresholds must be greater than 1")
    order, po = f.out(None, np.int16, "order") if grids is not None else (None, None)
    elev, pe = f.out(None, np.float32, "elevout") if grids is not None else (None, None)
    thresh, n1, n2 = np.zeros(nt, np.float32), np.zeros(nt, np.int64), np.zeros(nt, np.int64)
    sums, length = np.zeros((nt, 4), np.float64), np.zeros(nt, np.float64)
    head = (pa, pp, pf, ps, f.nx, f.ny, int(nodata), float(ssa_nodata), pdx, pdy)
    ladder = (ox, oy, no, float(thresh_min), float(thresh_max), nt, int(steptype), int(grids) if grids is not None else -1, po, pe, _v(thresh), _v(n1), _v(n2), _v(sums),
              _v(length))
    extra = () if grids is None else (order, elev)
    if f.strip:
        term = np.zeros(max(no, 1), np.float32)
        st = f.call("tdx_dropanalysis", *head, *ladder, _v(term))
        return (thresh, n1, n2, sums, length, term[:no]) + extra + (st,)
    dxc, dyc = f.keep[0], f.keep[1]
    scal, found = np.zeros(2, np.float32), np.zeros(1, np.int32)
    text = C.create_string_buffer(256 * nt + 512)
    st = f.call("tdx_dropanalysis", *head, abs(float(dxc[f.rows // 2])), abs(float(dyc[f.rows // 2])), *ladder, _v(scal[0:1]), _v(scal[1:2]), _v(found),
                C.cast(text, C.c_void_p), len(text))
    return (thresh, n1, n2, sums, length, scal[0], text.value.decode(), scal[1] if found[0] else None) + extra + (st,)


def _streamnet(f, p, src, fel, ad8, outlets, single_watershed, dx, dy, geotransform, nodata, src_nodata, out, phases, net=None, geographic=False, links="host"):
    if links not in _lib.STREAMNET_LINKS:
        raise ValueError(f"links: one of {_lib.STREAMNET_LINKS}, not {links!r}")
    pp = f.raster(p, np.int16, "p")
    ps = f.raster(src, np.int32, "src")
    pf = f.raster(fel, np.float32, "fel")
    pa = f.raster(ad8, np.float32, "ad8")
    pdx, pdy = f.cells(dx, dy)
    dxc, dyc = f.keep[0], f.keep[1]
    dxa, dya = abs(float(dxc[f.rows // 2])), abs(float(dyc[f.rows // 2]))
    gt = (0.0, dxa, 0.0, 0.0, 0.0, -dya) if geotransform is None else tuple(float(v) for v in geotransform)
    if len(gt) != 6:
        raise ValueError("geotransform: need GDAL's six numbers")
    g4 = np.array([gt[0], abs(gt[1]), gt[3], abs(gt[5])], np.float64)   # src/tiffIO.cpp:96-99
    if outlets is None:
        ox = oy = ids = np.zeros(0, np.int32)
    else:
        ox, oy = _flat(outlets[0], np.int32), _flat(outlets[1], np.int32)
        ids = _flat(outlets[2], np.int32) if len(outlets) > 2 else np.arange(1, ox.size + 1, dtype=np.int32)
        if ox.shape != oy.shape or ox.shape != ids.shape:
            raise ValueError("outlets: need equal-length 1-D arrays (columns, rows[, ids])")
    o_ord, o_w = out if out is not None else (None, None)
    ordg, po = f.out(o_ord, np.int16, "ord")
    w, pw = f.out(o_w, np.int32, "w")
    where, links = links, C.c_void_p()
    lib = f.ctx._lib
    st = f.call("tdx_streamnet" if where == "host" else "tdx_streamnet_gpu_links", pp, ps, pf, pa, f.nx, f.ny, int(nodata), int(src_nodata), pdx, pdy, dxa, dya, _v(g4), _v(ox) if ox.size else None,
                _v(oy) if ox.size else None, _v(ids) if ox.size else None, int(ox.size), int(bool(single_watershed)), po, pw, C.byref(links))
    try:
        tree, coord, ms = _links_rows(lib, links, phases=True)
        if net is not None:
            check(lib.tdx_streamnet_net_write(links, int(bool(geographic)), os.fsencode(net)))
    finally:
        lib.tdx_streamnet_links_free(links)
    res = (ordg, w, tree, coord)
    if phases:
        res += (ms,)
    return res + (st,)


def _links_rows(lib, links, phases=False):
    """(tree, coord[, phase dict]) of a tdx_streamnet_links handle; the dict of a device build holds the builder's own record as "links_device"."""
    npts = C.c_int64(0)
    nl = int(lib.tdx_streamnet_links_count(links, C.byref(npts), None))
    tree, coord, ms = np.empty((nl, 9), np.int64), np.empty((npts.value, 5), np.float64), np.zeros(len(_lib.STREAMNET_PHASES), np.float64)
    lib.tdx_streamnet_links_copy(links, _v(tree), _v(coord), _v(ms))
    if not phases:
        return tree, coord
    d = dict(zip(_lib.STREAMNET_PHASES, ms.tolist()))
    sub = _link_phases(lib, links)
    if sub is not None:
        d["links_device"] = sub
    return tree, coord, d


def _link_phases(lib, links):
    """The device link builder's record of a handle (tdx_streamnet_links_device_phases), None when the host built the links."""
    sub, jr, lr, wb = np.zeros(len(_lib.STREAMNET_LINK_PHASES), np.float64), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    if not lib.tdx_streamnet_links_device_phases(links, _v(sub), C.byref(jr), C.byref(lr), C.byref(wb)):
        return None
    return dict(zip(_lib.STREAMNET_LINK_PHASES, sub.tolist()), jump_rounds=jr.value, level_rounds=lr.value, workspace_bytes=wb.value)


def _streamnet_compact(f, p, src, fel, ad8, row0, dx, dy, nodata, src_nodata):
    """A strip's part of the stream cells (a handle: StreamNetLinks takes the parts of all strips) after the length sweep on the strip."""
    pp = f.raster(p, np.int16, "p")
    ps = f.raster(src, np.int32, "src")
    pf = f.raster(fel, np.float32, "fel")
    pa = f.raster(ad8, np.float32, "ad8")
    pdx, pdy = f.cells(dx, dy)
    part = C.c_void_p()
    st = f.call("tdx_streamnet_compact", pp, ps, pf, pa, f.nx, f.ny, int(row0), int(nodata), int(src_nodata), pdx, pdy, C.byref(part))
    return part, st


def _streamnet_label(f, p, src, part, links, first_cell, single_watershed, nodata, src_nodata):
    pp = f.raster(p, np.int16, "p")
    ps = f.raster(src, np.int32, "src")
    ordg, po = f.out(None, np.int16, "ord")
    w, pw = f.out(None, np.int32, "w")
    st = f.call("tdx_streamnet_label", pp, ps, f.nx, f.ny, int(nodata), int(src_nodata), part, links, int(first_cell), int(bool(single_watershed)), po, pw)
    return ordg, w, st


class StreamNetLinks:
    """The links of a raster from the parts of ALL its strips in strip order (StripPipeline.streamnet_compact): host code, no device - or with
    links="device" and a Context as ctx, built on that context's device (tdx_streamnet_links_build_gpu: the same bytes; link_phases then holds the
    builder's record).  tree / coord as Context.streamnet returns them; first_cell[k] is what strip k hands to StripPipeline.streamnet_label.  Owns the
    parts: close() frees them too."""

    def __init__(self, parts, nx, ny, dx, dy, geotransform=None, outlets=None, links="host", ctx=None):
        if links not in _lib.STREAMNET_LINKS:
            raise ValueError(f"links: one of {_lib.STREAMNET_LINKS}, not {links!r}")
        if links == "device" and ctx is None:
            raise ValueError('links="device" needs ctx, the Context whose device builds the links')
        self._lib = _lib.load()
        self.parts = list(parts)
        counts = [int(self._lib.tdx_streamnet_compact_count(p)) for p in self.parts]
        self.first_cell = [int(v) for v in np.concatenate([[0], np.cumsum(counts)[:-1]])]
        dxc, dyc = _f64(dx, ny), _f64(dy, ny)
        dxa, dya = abs(float(dxc[ny // 2])), abs(float(dyc[ny // 2]))
        gt = (0.0, dxa, 0.0, 0.0, 0.0, -dya) if geotransform is None else tuple(float(v) for v in geotransform)
        g4 = np.array([gt[0], abs(gt[1]), gt[3], abs(gt[5])], np.float64)
        if outlets is None:
            ox = oy = ids = np.zeros(0, np.int32)
        else:
            ox, oy = _flat(outlets[0], np.int32), _flat(outlets[1], np.int32)
            ids = _flat(outlets[2], np.int32) if len(outlets) > 2 else np.arange(1, ox.size + 1, dtype=np.int32)
        arr = (C.c_void_p * len(self.parts))(*[p.value for p in self.parts])
        self.handle = C.c_void_p()
        tail = (C.cast(arr, C.c_void_p), len(self.parts), int(nx), int(ny), dxa, dya, _v(g4), _v(ox) if ox.size else None, _v(oy) if ox.size else None,
                _v(ids) if ox.size else None, int(ox.size), C.byref(self.handle))
        if links == "device":
            check(self._lib.tdx_streamnet_links_build_gpu(ctx._h, *tail), ctx._h)
        else:
            check(self._lib.tdx_streamnet_links_build(*tail))
        self.tree, self.coord = _links_rows(self._lib, self.handle)
        self.link_phases = _link_phases(self._lib, self.handle)

    def write_net(self, path, geographic=False):
        """The stream network line layer of the links (tdx_streamnet_net_write): the file Context.streamnet(..., net=path) writes."""
        check(self._lib.tdx_streamnet_net_write(self.handle, int(bool(geographic)), os.fsencode(path)))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.tdx_streamnet_links_free(self.handle)
            self.handle = None
            for p in self.parts:
                self._lib.tdx_streamnet_compact_free(p)
            self.parts = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _rings_word(rings):
    if rings not in _lib.POLYGONIZE_RINGS:
        raise ValueError(f"rings: {rings!r} is neither 'host' nor 'device'")
    return rings


def _polygonize(f, w, nodata, rings="host"):
    symbol = "tdx_polygonize_gpu_rings" if _rings_word(rings) == "device" else "tdx_polygonize"
    pw = f.raster(w, np.int32, "w")
    handle = C.c_void_p()
    st = f.call(symbol, pw, f.nx, f.ny, int(nodata), C.byref(handle))
    return Polygons(handle=handle), st


def _polygonize_edges_strip(f, w, row0, ny_total, nodata):
    """A strip's part of the boundary edges (a handle: Polygons takes the parts of all strips).  The halo rows of w are the caller's: they hold the
    neighbouring strips' rows, are read, and are not written."""
    pw = f.raster(w, np.int32, "w")
    part = C.c_void_p()
    st = f.call("tdx_polygonize_edges", pw, f.nx, f.ny, int(row0), int(ny_total), int(nodata), C.byref(part))
    return part, st


def polygonize_edges(part):
    """keys, next_keys (int64) and ids (int32) of a part of boundary edges (StripPipeline.polygonize_edges)."""
    lib = _lib.load()
    n = int(lib.tdx_polygonize_edges_count(part))
    keys, nxt, ids = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
    lib.tdx_polygonize_edges_copy(part, _v(keys), _v(nxt), _v(ids), None)
    return keys, nxt, ids


def polygonize_edges_create(keys, next_keys, ids):
    """A part of boundary edges from arrays (host code): what drives the ring builder without a device."""
    lib = _lib.load()
    keys, nxt, ids = _flat(keys, np.int64), _flat(next_keys, np.int64), _flat(ids, np.int32)
    if not (keys.size == nxt.size == ids.size):
        raise ValueError("polygonize_edges_create: need three arrays of one length")
    part = C.c_void_p()
    n = int(keys.size)
    check(lib.tdx_polygonize_edges_create(_v(keys) if n else None, _v(nxt) if n else None, _v(ids) if n else None, n, C.byref(part)))
    return part


class Polygons:
    """The watershed polygons of an id grid: of Context.polygonize (handle=), or from the edge parts of ALL strips of a raster in strip order
    (parts=, nx=, ny=: StripPipeline.polygonize_edges; host code, no device - or with rings="device" and ctx=, a Context, closed on its device).  features -> polygons -> rings -> vertices as offset lists:
    ids int32 [F] ascending; cells int64 [F]; poly_first int64 [F + 1]; ring_first int64 [P + 1] (the outer ring of a polygon first, then its holes);
    vert_first int64 [R + 1]; vertices int32 [V, 2] (column, row), every ring closed; phases: the milliseconds of count, scan, emit, download, rings.
    ring_phases: the milliseconds of the device ring builder's sub-phases (empty when the host closed the rings), with ring_rounds (its jump rounds)
    and ring_workspace_bytes.
    Owns its handle and the parts: close() frees them."""

    def __init__(self, handle=None, parts=None, nx=None, ny=None, ctx=None, rings="host"):
        self._lib = _lib.load()
        _rings_word(rings)
        self.parts = list(parts) if parts is not None else []
        if handle is None:
            if not self.parts or nx is None or ny is None:
                raise ValueError("Polygons: need a handle, or parts with nx and ny")
            arr = (C.c_void_p * len(self.parts))(*[p.value for p in self.parts])
            handle = C.c_void_p()
            if rings == "device":
                if ctx is None:
                    raise ValueError("Polygons: rings='device' needs ctx=, the Context whose device closes the rings")
                check(self._lib.tdx_polygonize_rings_gpu(ctx._h, C.cast(arr, C.c_void_p), len(self.parts), int(nx), int(ny), C.byref(handle), None), ctx._h)
            else:
                check(self._lib.tdx_polygonize_rings(C.cast(arr, C.c_void_p), len(self.parts), int(nx), int(ny), C.byref(handle)))
        self.handle = handle
        lib = self._lib
        npoly, nring, nvert, nedge = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        nf = int(lib.tdx_polygons_count(handle, C.byref(npoly), C.byref(nring), C.byref(nvert), C.byref(nedge)))
        self.edges = int(nedge.value)
        self.ids, self.cells = np.zeros(nf, np.int32), np.zeros(nf, np.int64)
        self.poly_first, self.ring_first = np.zeros(nf + 1, np.int64), np.zeros(npoly.value + 1, np.int64)
        self.vert_first, self.vertices = np.zeros(nring.value + 1, np.int64), np.zeros((nvert.value, 2), np.int32)
        ms = np.zeros(len(_lib.POLYGONIZE_PHASES), np.float64)
        lib.tdx_polygons_copy(handle, _v(self.ids), _v(self.cells), _v(self.poly_first), _v(self.ring_first), _v(self.vert_first), _v(self.vertices), _v(ms))
        self.phases = dict(zip(_lib.POLYGONIZE_PHASES, ms.tolist()))
        rms, rounds, wsb = np.zeros(len(_lib.POLYGONIZE_RING_PHASES), np.float64), C.c_int64(0), C.c_int64(0)
        on_device = lib.tdx_polygons_ring_phases(handle, _v(rms), C.byref(rounds), C.byref(wsb))
        self.ring_phases = dict(zip(_lib.POLYGONIZE_RING_PHASES, rms.tolist())) if on_device else {}
        self.ring_rounds, self.ring_workspace_bytes = int(rounds.value), int(wsb.value)

    def features(self):
        """[(id, cells, [polygon, ...])] with polygon = [ring, ...] (the outer ring first) and ring = [(column, row), ...], closed."""
        out = []
        for f in range(self.ids.size):
            polys = []
            for p in range(self.poly_first[f], self.poly_first[f + 1]):
                polys.append([[tuple(int(v) for v in xy) for xy in self.vertices[self.vert_first[q]:self.vert_first[q + 1]]]
                              for q in range(self.ring_first[p], self.ring_first[p + 1])])
            out.append((int(self.ids[f]), int(self.cells[f]), polys))
        return out

    def write(self, path, geotransform=(0.0, 1.0, 0.0, 0.0, 0.0, -1.0)):
        """The polygon layer (tdx_polygons_write): ESRI shapefile or GeoJSON by the extension of path, x = gt[0] + column * gt[1], y = gt[3] + row * gt[5]."""
        gt = np.asarray([float(v) for v in geotransform], np.float64)
        if gt.size != 6:
            raise ValueError("geotransform: need GDAL's six numbers")
        check(self._lib.tdx_polygons_write(os.fsencode(path), self.handle, _v(gt)))

    def packed(self, geotransform=(0.0, 1.0, 0.0, 0.0, 0.0, -1.0)):
        """The features as PackedPolygons in map coordinates (x = gt[0] + column * gt[1], y = gt[3] + row * gt[5]): what Context.regiongrid burns back
        by the ids, without a file in between."""
        gt = [float(v) for v in geotransform]
        v = self.vertices.astype(np.float64)
        return PackedPolygons(gt[0] + v[:, 0] * gt[1], gt[3] + v[:, 1] * gt[5], self.vert_first, self.ring_first[self.poly_first])

    def close(self):
        if getattr(self, "handle", None):
            self._lib.tdx_polygons_free(self.handle)
            self.handle = None
            for p in self.parts:
                self._lib.tdx_polygonize_edges_free(p)
            self.parts = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def polygonize(w, nodata=-2147483647, device=0, *, rings="host", **kw):
    """Context(device).polygonize(...) for a single call; rings="device" closes the rings on the device (Context.polygonize_rings)."""
    _rings_word(rings)
    with Context(device) as ctx:
        return ctx.polygonize_rings(w, nodata, rings=rings, **kw) if rings != "host" else ctx.polygonize(w, nodata, **kw)


class PackedPolygons:
    """Polygons as the flat arrays the library takes, for layers too large for lists: x, y float64 [vertices]; ring_first int64 [rings + 1] (the vertices
    of a ring); feature_first int64 [features + 1] (the rings of a feature).  Context.regiongrid takes one as polygons=."""

    def __init__(self, x, y, ring_first, feature_first):
        self.x, self.y = _flat(x, np.float64), _flat(y, np.float64)
        self.ring_first, self.feature_first = _flat(ring_first, np.int64), _flat(feature_first, np.int64)
        if self.x.size != self.y.size or self.ring_first.size < 1 or self.feature_first.size < 1 or self.ring_first[-1] != self.x.size \
                or self.feature_first[-1] != self.ring_first.size - 1:
            raise ValueError("PackedPolygons: offsets that do not cover the vertices and rings")

    def __len__(self):
        return int(self.feature_first.size - 1)


def _pack_polygons(polygons, values):
    """x, y, ring_first, feature_first, values as the flat host arrays the library takes."""
    if isinstance(polygons, PackedPolygons):
        v64 = _flat(values, np.int64)
        if v64.size != len(polygons):
            raise ValueError("values: need one value per feature")
        lim = np.iinfo(np.int32)
        return polygons.x, polygons.y, polygons.ring_first, polygons.feature_first, np.ascontiguousarray(np.clip(v64, lim.min, lim.max).astype(np.int32))
    xs, ys, ring_first, feature_first = [], [], [0], [0]
    for feat in polygons:
        for ring in feat:
            r = np.asarray(ring, np.float64).reshape(-1, 2)
            xs.append(r[:, 0])
            ys.append(r[:, 1])
            ring_first.append(ring_first[-1] + r.shape[0])
        feature_first.append(len(ring_first) - 1)
    x = np.ascontiguousarray(np.concatenate(xs)) if xs else np.zeros(0, np.float64)
    y = np.ascontiguousarray(np.concatenate(ys)) if ys else np.zeros(0, np.float64)
    v64 = _flat(values, np.int64)
    if v64.size != len(feature_first) - 1:
        raise ValueError("values: need one value per feature")
    lim = np.iinfo(np.int32)   # a value beyond int32 is for the library to refuse: it keeps that meaning after the clip
    return x, y, np.asarray(ring_first, np.int64), np.asarray(feature_first, np.int64), np.ascontiguousarray(np.clip(v64, lim.min, lim.max).astype(np.int32))


def _gt6(gt, name):
    g = np.ascontiguousarray(np.asarray([float(v) for v in gt], np.float64))
    if g.size != 6:
        raise ValueError(f"{name}: need GDAL's six numbers")
    return g


def _regiongrid(f, shape, gt, polygons, values, source, source_gt, source_nodata, out, workspace_words=0, row0=None, ny_total=None, phases=False):
    """row0, ny_total: a strip's first owned row and the raster's rows (gt is the whole raster's); None for a Context.  phases: ask for the phase times."""
    if polygons is not None and source is not None:
        raise ValueError("regiongrid: polygons and source exclude each other")
    g = _gt6(gt, "gt")
    f.keep.append(g)
    if not f.strip:
        ny, nx = (int(v) for v in shape)
        if nx <= 0 or ny <= 0:
            raise ValueError("shape: need (ny, nx) > 0")
        f.shape = (ny, nx)
    if out is None:
        if f.strip or _is_torch(source):
            import torch

            out = torch.empty(f.shape, dtype=torch.int16, device=f"cuda:{f.ctx.device}")
        else:
            out = np.empty(f.shape, np.int16)
    po = f.raster(out, np.int16, "out")
    where = (f.nx, f.ny) if row0 is None else (f.nx, f.ny, int(row0), int(ny_total))
    ids, n_ids = np.zeros(_lib.REGIONGRID_MAX_IDS, np.int32), C.c_int32(0)
    ms, ws = np.zeros(len(_lib.REGIONGRID_PHASES), np.float64), C.c_int64(0)
    pms = _v(ms) if phases else None
    if polygons is not None:
        if values is None:
            raise ValueError("regiongrid: polygons need values")
        x, y, ring_first, feature_first, vals = _pack_polygons(polygons, values)
        f.keep += [x, y, ring_first, feature_first, vals]
        st = f.call("tdx_regiongrid", _v(x) if x.size else None, _v(y) if y.size else None, _v(ring_first), int(ring_first.size - 1), _v(feature_first),
                    _v(vals) if vals.size else None, int(vals.size), _v(g), int(workspace_words), *where, po, _v(ids), C.byref(n_ids), pms, C.byref(ws))
    elif source is not None:
        if source_gt is None:
            raise ValueError("regiongrid: source needs source_gt")
        sg = _gt6(source_gt, "source_gt")
        dev = _is_torch(source)
        if dev != f.dev:
            raise ValueError("source: all rasters must be on the same side (host or device)")
        if dev:
            if not source.is_cuda or source.device.index != f.ctx.device or source.dtype != _torch_dtype(np.int32) or not source.is_contiguous() or source.dim() != 2:
                raise ValueError(f"source: need a contiguous 2-D int32 tensor on cuda:{f.ctx.device}")
            ps = C.c_void_p(source.data_ptr())
        else:
            if not isinstance(source, np.ndarray) or source.dtype != np.int32 or not source.flags.c_contiguous or source.ndim != 2:
                raise ValueError("source: need a C-contiguous 2-D numpy int32 array")
            ps = C.c_void_p(source.ctypes.data)
        sny, snx = (int(v) for v in source.shape)
        f.keep += [sg, source]
        st = f.call("tdx_regiongrid_resample", ps, snx, sny, _v(sg), int(source_nodata), _v(g), *where, po, _v(ids), C.byref(n_ids), pms)
    else:
        st = f.call("tdx_regiongrid_constant", *where, po, _v(ids), C.byref(n_ids))
    if phases:
        st["phases"] = dict(zip(_lib.REGIONGRID_PHASES, ms.tolist()))
    st["workspace_bytes"] = int(ws.value)
    return out, ids[:n_ids.value].copy(), st


def regiongrid(shape, gt, polygons=None, values=None, source=None, source_gt=None, source_nodata=-2147483647, device=0, **kw):
    """Context(device).regiongrid(...) for a single call."""
    with Context(device) as ctx:
        return ctx.regiongrid(shape, gt, polygons, values, source, source_gt, source_nodata, **kw)


class PolygonLayer:
    """A polygon layer read from a file (read_polygons): polygons - a list of features, each a list of rings, each a float64 (n, 2) array of x, y, what
    Context.regiongrid takes; fields - {name: [text per feature]} with "" for a null; values(field) - the region ids of a field, checked by the
    library.  It owns a handle of the library: close() it or use it as a context manager (the arrays stay valid afterwards; values() does not)."""

    def __init__(self, handle):
        lib = self._lib = _lib.load()
        self.handle = handle
        nr, nv, nf = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        n = int(lib.tdx_polygon_layer_count(handle, C.byref(nr), C.byref(nv), C.byref(nf)))
        feature_first, ring_first = np.zeros(n + 1, np.int64), np.zeros(nr.value + 1, np.int64)
        xy = np.zeros((2, max(nv.value, 1)), np.float64)
        lib.tdx_polygon_layer_copy(handle, _v(feature_first), _v(ring_first), _v(xy[0]), _v(xy[1]))
        pts = np.ascontiguousarray(xy[:, :nv.value].T)
        self.polygons = [[pts[ring_first[q]:ring_first[q + 1]] for q in range(feature_first[f], feature_first[f + 1])] for f in range(n)]
        names = [lib.tdx_polygon_layer_field(handle, k).decode() for k in range(nf.value)]
        self.fields = {name: [(lib.tdx_polygon_layer_value(handle, f, k) or b"").decode(errors="replace").strip(" \0") for f in range(n)] for k, name in enumerate(names)}

    def values(self, field="ID"):
        """int32 per feature: the integer values of `field`, each in 1 .. 32767 (tdx_polygon_layer_values).  TdxError naming the feature: no such field,
        the field name FID, a null, a value that is no integer, a value outside the range."""
        if not self.handle:
            raise ValueError("PolygonLayer.values: the layer is closed")
        v = np.zeros(max(len(self.polygons), 1), np.int32)
        check(self._lib.tdx_polygon_layer_values(self.handle, os.fsencode(field), _v(v)))
        return v[:len(self.polygons)].copy()

    def close(self):
        if getattr(self, "handle", None):
            self._lib.tdx_polygon_layer_free(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()

    def __len__(self):
        return len(self.polygons)


def read_polygons(path):
    """The polygon layer of an ESRI shapefile (shape types 5, 15, 25 with the .dbf beside it; Z and M ignored) or of a GeoJSON file (Polygon and
    MultiPolygon features in document order): a PolygonLayer.  Every part is a ring; nesting is not rebuilt, the even-odd fill of regiongrid does not
    need it.  No GPU is needed.  TdxError: an unsupported extension, an unreadable file, or one whose headers, lengths, counts or part indices lie."""
    h = C.c_void_p()
    check(_lib.load().tdx_polygon_layer_read(os.fsencode(path), C.byref(h)))
    return PolygonLayer(h)


def write_calpar(path, ids, tmin=2.708, tmax=2.708, cmin=0.0, cmax=0.25, phimin=30.0, phimax=45.0, soildens=2000.0):
    """The region table sinmapsi reads as -calpar: the header line, then id,tmin,tmax,cmin,cmax,phimin,phimax,soildens per id in the order given, the
    seven parameters as repr(float(value)) (the defaults are those of pyfiles/SIRegionTool.py).  No GPU is needed; read_calpar() reads the file back."""
    lib = _lib.load()
    ids = _flat(ids, np.int32)
    texts = [repr(float(v)).encode() for v in (tmin, tmax, cmin, cmax, phimin, phimax, soildens)]
    arr = (C.c_char_p * 7)(*texts)
    check(lib.tdx_regiongrid_write_calpar(os.fsencode(path), _v(ids) if ids.size else None, int(ids.size), C.cast(arr, C.c_void_p)))


def _point_lists(outlets):
    ox, oy = _flat(outlets[0], np.int32).copy(), _flat(outlets[1], np.int32).copy()
    if ox.shape != oy.shape:
        raise ValueError("outlets: need two equal-length 1-D index arrays (columns, rows)")
    return ox, oy


def _moveoutlets(f, p, src, outlets, maxdist, nodata, src_nodata):
    pp = f.raster(p, np.int16, "p")
    ps = f.raster(src, np.int32, "src")
    ox, oy = _point_lists(outlets)
    rx, ry, rd = np.zeros_like(ox), np.zeros_like(ox), np.zeros_like(ox)
    n = int(ox.size)
    st = f.call("tdx_moveoutlets", pp, ps, f.nx, f.ny, int(nodata), int(src_nodata), int(maxdist), _v(ox) if n else None, _v(oy) if n else None, n,
                _v(rx) if n else None, _v(ry) if n else None, _v(rd) if n else None)
    return rx, ry, rd, st


def _moveoutlets_strip(f, p, src, row0, ny_total, maxdist, state, nodata, src_nodata):
    """state = (columns, global rows, dist, done): int32 arrays advanced in place; returns the number of outlets this strip advanced or finished."""
    pp = f.raster(p, np.int16, "p")
    ps = f.raster(src, np.int32, "src")
    sx, sy, sd, sn = _walk_state(state)
    moved = C.c_int64(0)
    n = int(sx.size)
    st = f.call("tdx_moveoutlets", pp, ps, f.nx, f.ny, int(row0), int(ny_total), int(nodata), int(src_nodata), int(maxdist), _v(sx) if n else None,
                _v(sy) if n else None, _v(sd) if n else None, _v(sn) if n else None, n, C.byref(moved))
    return int(moved.value), st


def _walk_state(state):
    for a in state:
        if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.ndim != 1 or not a.flags.c_contiguous or a.shape != state[0].shape:
            raise ValueError("state: need equal-length C-contiguous 1-D int32 numpy arrays")
    return state


def _points_rows(lib, points, phases=False):
    """The seven arrays of a tdx_connectdown_points handle (and the phase dict)."""
    n = int(lib.tdx_connectdown_points_count(points))
    ids, x, y, mx, my, down = (np.zeros(n, np.int32) for _ in range(6))
    amax, ms = np.zeros(n, np.float32), np.zeros(len(_lib.CONNECTDOWN_PHASES), np.float64)
    lib.tdx_connectdown_points_copy(points, _v(ids), _v(x), _v(y), _v(amax), _v(mx), _v(my), _v(down), _v(ms))
    res = (ids, x, y, amax, mx, my, down)
    return res + (dict(zip(_lib.CONNECTDOWN_PHASES, ms.tolist())),) if phases else res


def _connectdown(f, p, w, ad8, movedist, nodata, w_nodata, phases):
    pp = f.raster(p, np.int16, "p")
    pw = f.raster(w, np.int32, "w")
    pa = f.raster(ad8, np.float32, "ad8")
    points = C.c_void_p()
    lib = f.ctx._lib
    st = f.call("tdx_connectdown", pp, pw, pa, f.nx, f.ny, int(nodata), int(w_nodata), int(movedist), C.byref(points))
    try:
        res = _points_rows(lib, points, phases)
    finally:
        lib.tdx_connectdown_points_free(points)
    return res + (st,)


def _connectdown_strip(f, w, ad8, row0, w_nodata):
    """A strip's part of the maxima (a handle: ConnectDownPoints takes the parts of all strips)."""
    pw = f.raster(w, np.int32, "w")
    pa = f.raster(ad8, np.float32, "ad8")
    part = C.c_void_p()
    st = f.call("tdx_connectdown", pw, pa, f.nx, f.ny, int(row0), int(w_nodata), C.byref(part))
    return part, st


def _connectdown_walk_strip(f, p, w, row0, ny_total, movedist, state):
    """state = (columns, global rows, dist, done, id_down), advanced in place; returns the number of points this strip advanced or finished."""
    pp = f.raster(p, np.int16, "p")
    pw = f.raster(w, np.int32, "w")
    sx, sy, sd, sn, si = _walk_state(state)
    moved = C.c_int64(0)
    n = int(sx.size)
    st = f.call("tdx_connectdown_walk", pp, pw, f.nx, f.ny, int(row0), int(ny_total), int(movedist), _v(sx) if n else None, _v(sy) if n else None,
                _v(sd) if n else None, _v(sn) if n else None, _v(si) if n else None, n, C.byref(moved))
    return int(moved.value), st


class ConnectDownPoints:
    """The maxima of a raster from the parts of ALL its strips in strip order (StripPipeline.connectdown_argmax): host code, no device.  ids, columns,
    rows (of the whole raster) and ad8max as Context.connectdown returns them; state() is what the strips' connectdown_walk is handed, and
    moved(state) the three arrays that complete Context.connectdown's result.  Owns the parts: close() frees them."""

    def __init__(self, parts):
        self._lib = _lib.load()
        self.parts = list(parts)
        arr = (C.c_void_p * len(self.parts))(*[p.value for p in self.parts])
        self.handle = C.c_void_p()
        check(self._lib.tdx_connectdown_merge(C.cast(arr, C.c_void_p), len(self.parts), C.byref(self.handle)))
        self.ids, self.columns, self.rows, self.ad8max = _points_rows(self._lib, self.handle)[:4]

    def state(self):
        n = self.ids.size
        return self.columns.copy(), self.rows.copy(), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)

    @staticmethod
    def moved(state):
        return state[0], state[1], state[4]

    def close(self):
        if getattr(self, "handle", None):
            self._lib.tdx_connectdown_points_free(self.handle)
            self.handle = None
            for p in self.parts:
                self._lib.tdx_connectdown_points_free(p)
            self.parts = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def moveoutletstostrm(p, src, outlets, maxdist=50, device=0, **kw):
    """Context(device).moveoutletstostrm(...) for a single call."""
    with Context(device) as ctx:
        return ctx.moveoutletstostrm(p, src, outlets, maxdist, **kw)


def connectdown(p, w, ad8, movedist=10, device=0, **kw):
    """Context(device).connectdown(...) for a single call."""
    with Context(device) as ctx:
        return ctx.connectdown(p, w, ad8, movedist, **kw)


def write_points(path, x, y, fields=None):
    """A point layer at `path`: an ESRI shapefile (.shp, with its .shx and .dbf) or GeoJSON (.json / .geojson) by the extension; any other raises.
    fields: {name: values}, one value per point; integer arrays become Integer fields, floating ones Real, anything else String.  Host code: needs
    no GPU.  No .prj is written."""
    xs, ys = _flat(x, np.float64), _flat(y, np.float64)
    if xs.shape != ys.shape:
        raise ValueError("x and y: need equal-length arrays")
    n = int(xs.size)
    k, c_names, c_types, c_cols, keep = _field_columns(fields, n)
    check(_lib.load().tdx_points_write(str(path).encode(), _v(xs) if n else None, _v(ys) if n else None, n, k, C.cast(c_names, C.c_void_p) if k else None,
                                       _v(c_types) if k else None, C.cast(c_cols, C.c_void_p) if k else None))


def _field_columns(fields, n):
    """(count, names, types, columns, what keeps them alive) of {name: values} for tdx_points_write / tdx_lines_write"""
    names, types, cols, keep = [], [], [], []
    for name, vals in dict(fields or {}).items():
        a = np.asarray(vals)
        if a.shape != (n,):
            raise ValueError(f"field {name}: need one value per feature")
        if a.dtype.kind in "iub":
            if a.size and (a.min() < -2**31 or a.max() > 2**31 - 1):
                raise ValueError(f"field {name}: integers beyond 32 bits")
            a, t = np.ascontiguousarray(a, np.int32), 0
            ptr = a.ctypes.data
        elif a.dtype.kind == "f":
            a, t = np.ascontiguousarray(a, np.float64), 1
            ptr = a.ctypes.data
        else:
            strs = [str(v).encode() for v in a.tolist()]
            a, t = (C.c_char_p * max(n, 1))(*strs), 2
            ptr = C.cast(a, C.c_void_p).value
        names.append(str(name).encode()); types.append(t); cols.append(ptr); keep.append(a)
    k = len(names)
    return k, (C.c_char_p * max(k, 1))(*names), np.array(types + [0], np.int32), (C.c_void_p * max(k, 1))(*cols), keep


def _line_arrays(lines):
    """first (n + 1 offsets), x, y of a list of (vertices, 2) arrays"""
    parts = [np.asarray(v, np.float64).reshape(-1, 2) for v in lines]
    first = np.zeros(len(parts) + 1, np.int64)
    if parts:
        first[1:] = np.cumsum([len(v) for v in parts])
    xy = np.concatenate(parts, axis=0) if parts else np.zeros((0, 2), np.float64)
    return first, np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])


def write_lines(path, lines, fields=None, widths=None):
    """A line layer at `path`: an ESRI shapefile (.shp of PolyLines, one part each, with its .shx and .dbf) or GeoJSON (LineString features) by the
    extension; any other raises.  lines: one (vertices, 2) array of x, y per feature - a single vertex is legal; fields: {name: values} as for
    write_points; widths: {name: (width, decimals)} for the .dbf columns (streamnet_net's fields come with theirs: api.NET_WIDTHS).  Host code: needs
    no GPU.  No .prj is written."""
    first, xs, ys = _line_arrays(lines)
    n = len(first) - 1
    k, c_names, c_types, c_cols, keep = _field_columns(fields, n)
    wd = np.zeros((2, max(k, 1)), np.int32)
    for j, name in enumerate(dict(fields or {})):
        wd[:, j] = (widths or {}).get(name, (0, 0))
    check(_lib.load().tdx_lines_write(str(path).encode(), _v(first), _v(xs) if xs.size else None, _v(ys) if xs.size else None, n, k,
                                      C.cast(c_names, C.c_void_p) if k else None, _v(c_types) if k else None, _v(wd[0]) if k else None, _v(wd[1]) if k else None,
                                      C.cast(c_cols, C.c_void_p) if k else None))


def read_lines(path):
    """lines, fields of a line layer (shapefile PolyLine / PolyLineZ / PolyLineM, or GeoJSON LineString features): one (vertices, 2) float64 array per
    feature, and {name: values} with int32 arrays for Integer fields, float64 for Real ones (a null is 0), lists of str for the rest.  Host code."""
    lib = _lib.load()
    h = C.c_void_p()
    check(lib.tdx_lines_read(str(path).encode(), C.byref(h)))
    try:
        nv, nf = C.c_int64(0), C.c_int32(0)
        n = int(lib.tdx_line_layer_count(h, C.byref(nv), C.byref(nf)))
        first, x, y = np.zeros(n + 1, np.int64), np.zeros(nv.value, np.float64), np.zeros(nv.value, np.float64)
        lib.tdx_line_layer_vertices(h, _v(first), _v(x), _v(y))
        lines = [np.stack([x[a:b], y[a:b]], axis=1) for a, b in zip(first[:-1], first[1:])]
        fields = {}
        for k in range(nf.value):
            t = C.c_int32(0)
            name = lib.tdx_line_layer_field(h, k, C.byref(t), None, None).decode()
            text = [lib.tdx_line_layer_value(h, i, k).decode("utf-8", "replace").strip(" \0") for i in range(n)]
            if t.value == 2:
                fields[name] = text
            else:
                fields[name] = np.array([float(v) if v else 0.0 for v in text], np.float64)
                if t.value == 0:
                    fields[name] = fields[name].astype(np.int32)
        return lines, fields
    finally:
        lib.tdx_line_layer_free(h)


NET_WIDTHS = {name: (w, d) for name, _, w, d in _lib.NET_FIELDS}


def streamnet_net(tree, coord, geographic=False):
    """fields, lines = the stream network layer of Context.streamnet's tree and coord rows (reachshape(), src/streamnet.cpp:244-365): the 17 fields of
    the reference's -net layer as {name: array} in its order (int32 / float64), and per link its (vertices, 2) array, REVERSED so that vertex 0 is the
    downstream end; a link of one point is a line of one vertex.  geographic: the raster's flag (every segment's length is then tiffIO::geotoLength's).
    write_lines(path, lines, fields, NET_WIDTHS) writes what tdx_streamnet_net_write does.  Host code: needs no GPU."""
    tree = np.ascontiguousarray(np.asarray(tree, np.int64).reshape(-1, 9))
    coord = np.ascontiguousarray(np.asarray(coord, np.float64).reshape(-1, 5))
    nl = len(tree)
    nv = int((tree[:, 2] - tree[:, 1] + 1).sum()) if nl else 0
    real, first = np.zeros((nl, 9), np.float64), np.zeros(nl + 1, np.int64)
    x, y = np.zeros(max(nv, 0), np.float64), np.zeros(max(nv, 0), np.float64)
    check(_lib.load().tdx_streamnet_net_rows(_v(tree), _v(coord), nl, len(coord), int(bool(geographic)), nv, _v(real), _v(first), _v(x), _v(y)))
    fields, r = {}, 0
    for name, t, _, _ in _lib.NET_FIELDS:
        if t == 0:
            fields[name] = tree[:, _lib.NET_TREE_COLUMN[name]].astype(np.int32)
        else:
            fields[name] = real[:, r].copy()
            r += 1
    return fields, [np.stack([x[a:b], y[a:b]], axis=1) for a, b in zip(first[:-1], first[1:])]


def catchoutlets(pfile, fields, lines, mindist=0.0, gwstartno=1, minarea=0.0):
    """x, y, fields = CatchOutlets (src/CatchOutlets.cpp:126) on the stream network (fields, lines) - streamnet_net's or read_lines' - and the D8 flow
    direction FILE pfile, of which the header and one cell per outlet link are read: the outlets in the reference's order with the fields LINKNO,
    DSLINKNO, USLINKNO1, USLINKNO2, DOUTEND and Id of its point layer (write_points(path, x, y, fields) writes it).  Vertex 0 of a line is the link's
    downstream end.  Host code: no context is created and no GPU touched."""
    need = ("LINKNO", "DSLINKNO", "USLINKNO1", "USLINKNO2", "DOUTEND", "DOUTSTART", "USContArea")
    for name in need:
        if name not in fields:
            raise ValueError(f"the stream network has no field {name}")
    n = len(lines)
    ints = [np.ascontiguousarray(np.asarray(fields[k]), np.int32) for k in need[:4]]
    reals = [np.ascontiguousarray(np.asarray(fields[k]), np.float64) for k in need[4:]]
    if any(a.shape != (n,) for a in ints + reals):
        raise ValueError("need one value per line in every field")
    ends = np.zeros((4, n), np.float64)
    for i, v in enumerate(lines):
        v = np.asarray(v, np.float64).reshape(-1, 2)
        if len(v):
            ends[:, i] = (v[0, 0], v[0, 1], v[-1, 0], v[-1, 1])
        elif ints[1][i] < 0 or ints[2][i] >= 0 or ints[3][i] >= 0:
            raise ValueError(f"line {i} has no vertex")
    cap = 2 * n + 2
    row, ox, oy, od, oid, nout = np.zeros(cap, np.int64), np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(cap, np.int32), C.c_int64(0)
    check(_lib.load().tdx_catchoutlets(os.fsencode(pfile), *[_v(a) for a in ints], *[_v(a) for a in reals], *[_v(np.ascontiguousarray(e)) for e in ends], n,
                                       float(mindist), int(gwstartno), float(minarea), cap, _v(row), _v(ox), _v(oy), _v(od), _v(oid), C.byref(nout)))
    m = nout.value
    row = row[:m]
    out = {k: a[row] for k, a in zip(need[:4], ints)}
    out["DOUTEND"], out["Id"] = od[:m].copy(), oid[:m].copy()
    return ox[:m].copy(), oy[:m].copy(), out


def streamnet_text(tree, coord):
    """The bytes of the reference's -tree and -coord files (src/streamnet.cpp:1165, :1177) from Context.streamnet's rows."""
    t = "".join("\t" + "\t".join(str(int(v)) for v in row) + "\n" for row in np.asarray(tree, np.int64).reshape(-1, 9))
    c = "".join("\t%f\t%f\t%f\t%f\t%f\n" % tuple(float(v) for v in row) for row in np.asarray(coord, np.float64).reshape(-1, 5))
    return t.encode(), c.encode()


def streamnet(p, src, fel, ad8, outlets=None, single_watershed=False, device=0, **kw):
    """Context(device).streamnet(...) for a single call."""
    with Context(device) as ctx:
        return ctx.streamnet(p, src, fel, ad8, outlets, single_watershed, **kw)


def dropanalysis_table(thresh, n1, n2, s1, s1sq, s2, s2sq, length, total_area):
    """table, console, optimum = the table file and the console lines of DropAnalysis (src/DropAnalysis.cpp:597-674) from the float sums of all
    thresholds, with the reference's own float / double expressions; optimum None when no threshold qualifies.  Host code: needs no GPU."""
    thresh, s1, s1sq, s2, s2sq = (_flat(a, np.float32) for a in (thresh, s1, s1sq, s2, s2sq))
    n1, n2, length = _flat(n1, np.int64), _flat(n2, np.int64), _flat(length, np.float64)
    nt = thresh.size
    if any(a.size != nt for a in (n1, n2, s1, s1sq, s2, s2sq, length)):
        raise ValueError("dropanalysis_table: need one entry per threshold in every array")
    table, console = C.create_string_buffer(256 * nt + 512), C.create_string_buffer(256 * nt + 1024)
    opt, found = C.c_float(0.0), C.c_int32(0)
    check(_lib.load().tdx_dropanalysis_table(nt, _v(thresh), _v(n1), _v(n2), _v(s1), _v(s1sq), _v(s2), _v(s2sq), _v(length), float(total_area), C.cast(table, C.c_void_p),
                                             len(table), C.cast(console, C.c_void_p), len(console), C.byref(opt), C.byref(found)))
    return table.value.decode(), console.value.decode(), np.float32(opt.value) if found.value else None


def dropanalysis(ad8, p, fel, ssa, outlets, device=0, **kw):
    """Context(device).dropanalysis(...) for a single call."""
    with Context(device) as ctx:
        return ctx.dropanalysis(ad8, p, fel, ssa, outlets, **kw)


def peukerdouglas(fel, device=0, **kw):
    """Context(device).peukerdouglas(...) for a single call."""
    with Context(device) as ctx:
        return ctx.peukerdouglas(fel, **kw)


def terrain_indices(slp, sca, m=2.0, n=1.0, want=_lib.TERRAIN_OUTPUTS, device=0, **kw):
    """Context(device).terrain_indices(...) for a single call."""
    with Context(device) as ctx:
        return ctx.terrain_indices(slp, sca, m, n, want, **kw)


def lengtharea(plen, ad8, M=0.03, y=1.3, device=0, **kw):
    """Context(device).lengtharea(...) for a single call."""
    with Context(device) as ctx:
        return ctx.lengtharea(plen, ad8, M, y, **kw)


def setregion(p, gw, region_id=1, device=0, **kw):
    """Context(device).setregion(...) for a single call."""
    with Context(device) as ctx:
        return ctx.setregion(p, gw, region_id, **kw)


def editraster(raster, cols, rows, vals, device=0, **kw):
    """Context(device).editraster(...) for a single call."""
    with Context(device) as ctx:
        return ctx.editraster(raster, cols, rows, vals, **kw)


def sinmapsi(slp, sca, cal, regions, rminter, rmaxter, g=9.81, rhow=1000.0, device=0, **kw):
    """Context(device).sinmapsi(...) for a single call."""
    with Context(device) as ctx:
        return ctx.sinmapsi(slp, sca, cal, regions, rminter, rmaxter, g, rhow, **kw)


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
