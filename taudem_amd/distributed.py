"""Row strips across GPUs: one process per GPU, one horizontal strip (+ one halo row above and below)
per process - the layout of the reference's linearpart<T> (src/linearpart.h:133-162) - with the halo
exchange and the termination votes carried by torch.distributed (backend "nccl" = RCCL over xGMI on a
GPU node; "gloo" with host staging for CPU-side tests and for several ranks sharing one GPU).

The library itself never talks to a communication library: it calls back into :class:`StripComm`
through the ``tdx_comm`` struct of include/taudem_amd.h (exchange one boundary row with each strip
neighbour; all-reduce a few int64 on the host).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, api
from ._lib import check
from .api import ANG_NODATA, FEL_NODATA, P_NODATA


def partition_rows(ny: int, size: int):
    """Row ranges [y0, y1) per rank: ny // size rows each, the remainder to the last rank
    (src/linearpart.h:133-134)."""
    base = ny // size
    out = []
    for r in range(size):
        y0 = r * base
        y1 = (r + 1) * base if r < size - 1 else ny
        out.append((y0, y1))
    return out


def strip_rows(per_row, y0: int, y1: int):
    """Global per-row values (cell sizes dxc / dyc of ny rows) -> the y1 - y0 + 2 rows of the strip array of [y0, y1): the halo rows
    are the global rows y0 - 1 and y1, clamped into the raster (rows_of in taudem_amd/csrc/tool_strips.hpp).  A scalar stays a scalar.
    The clamp is the 1-rank reference: a strip's edge cells read the neighbouring global row, whatever the cut."""
    a = np.asarray(per_row, dtype=np.float64)
    if a.ndim == 0:
        return float(a)
    ny = a.shape[0]
    if not (0 <= y0 < y1 <= ny):
        raise ValueError(f"strip rows [{y0}, {y1}) outside the {ny} rows given")
    return np.ascontiguousarray(a[np.clip(np.arange(y0 - 1, y1 + 1), 0, ny - 1)])


class StripComm:
    """tdx_comm backed by a torch.distributed process group (ranks ordered north to south)."""

    def __init__(self, nx: int, device: int | None = 0, group=None):
        """device=None keeps the four exchange buffers in host memory (protocol tests without a GPU)."""
        import torch
        import torch.distributed as dist

        self.torch, self.dist, self.group = torch, dist, group
        self.rank = dist.get_rank(group)
        self.size = dist.get_world_size(group)
        self.backend = dist.get_backend(group)
        self.dev = torch.device(f"cuda:{device}") if device is not None else torch.device("cpu")
        self.capacity = 16 * int(nx)
        self._bufs = [torch.zeros(self.capacity, dtype=torch.uint8, device=self.dev) for _ in range(4)]   # send_up send_down recv_up recv_down
        self._host = None
        if self.backend != "nccl" and self.dev.type == "cuda":
            self._host = [torch.zeros(self.capacity, dtype=torch.uint8).pin_memory() for _ in range(4)]
        self.exchanges = 0
        self.allreduces = 0
        self._ex_cb = _lib.EXCHANGE_FN(self._exchange)
        self._ar_cb = _lib.ALLREDUCE_FN(self._allreduce)
        self.struct = _lib.TdxComm(self.rank, self.size, None, self._ex_cb, self._ar_cb, *[C.c_void_p(b.data_ptr()) for b in self._bufs], self.capacity)

    def ptr(self):
        return C.byref(self.struct)

    def _peer(self, delta):
        r = self.rank + delta
        if r < 0 or r >= self.size:
            return None
        return self.dist.get_global_rank(self.group, r) if self.group is not None else r

    def _exchange(self, user, nbytes):
        try:
            torch, dist = self.torch, self.dist
            n = int(nbytes)
            up, down = self._peer(-1), self._peer(+1)
            self.exchanges += 1
            if self.backend == "nccl":
                s_up, s_dn, r_up, r_dn = [b[:n] for b in self._bufs]
                ops = []
                if up is not None:
                    ops += [dist.P2POp(dist.isend, s_up, up, self.group), dist.P2POp(dist.irecv, r_up, up, self.group)]
                if down is not None:
                    ops += [dist.P2POp(dist.isend, s_dn, down, self.group), dist.P2POp(dist.irecv, r_dn, down, self.group)]
                if ops:
                    for w in dist.batch_isend_irecv(ops):
                        w.wait()
                torch.cuda.synchronize(self.dev)
            else:   # gloo: host staging (or host buffers to begin with)
                staged = self._host is not None
                h = [x[:n] for x in (self._host if staged else self._bufs)]
                if staged:
                    if up is not None:
                        h[0].copy_(self._bufs[0][:n])
                    if down is not None:
                        h[1].copy_(self._bufs[1][:n])
                    torch.cuda.synchronize(self.dev)
                reqs = []
                if up is not None:
                    reqs += [dist.isend(h[0], up, self.group, tag=1), dist.irecv(h[2], up, self.group, tag=2)]
                if down is not None:
                    reqs += [dist.isend(h[1], down, self.group, tag=2), dist.irecv(h[3], down, self.group, tag=1)]
                for r in reqs:
                    r.wait()
                if staged:
                    if up is not None:
                        self._bufs[2][:n].copy_(h[2])
                    if down is not None:
                        self._bufs[3][:n].copy_(h[3])
                    torch.cuda.synchronize(self.dev)
            return 0
        except Exception as e:   # never let an exception cross the C boundary
            import sys
            print(f"StripComm.exchange failed on rank {self.rank}: {e!r}", file=sys.stderr, flush=True)
            return 1

    def _allreduce(self, user, values, count, op):
        try:
            torch, dist = self.torch, self.dist
            self.allreduces += 1
            a = np.ctypeslib.as_array(values, shape=(int(count),))
            t = torch.from_numpy(a.copy())
            if self.backend == "nccl":
                t = t.to(self.dev)
            dist.all_reduce(t, op=dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MAX, group=self.group)
            a[:] = t.cpu().numpy()
            return 0
        except Exception as e:
            import sys
            print(f"StripComm.allreduce failed on rank {self.rank}: {e!r}", file=sys.stderr, flush=True)
            return 1


class RcclStripComm:
    """tdx_comm backed by the library's NATIVE RCCL transport (taudem_amd/csrc/comm.cpp): boundary rows travel as grouped
    ncclSend/ncclRecv on the context's stream, termination votes as ncclAllReduce on device values - no Python, no host
    staging and no extra synchronisation in the exchange path.  torch.distributed is only the bootstrap: rank 0's
    ncclUniqueId is broadcast through the process group (any backend) once."""

    def __init__(self, ctx, nx: int, group=None):
        import torch
        import torch.distributed as dist

        self.ctx = ctx
        self._lib = ctx._lib
        self.rank = dist.get_rank(group)
        self.size = dist.get_world_size(group)
        ident = (C.c_ubyte * 128)()
        if self.rank == 0:
            check(self._lib.tdx_rccl_unique_id(ident))
        box = [bytes(ident)]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        ident = (C.c_ubyte * 128).from_buffer_copy(box[0])
        h = C.c_void_p()
        check(self._lib.tdx_rccl_comm_create(ctx._h, ident, self.rank, self.size, int(nx), C.byref(h)), ctx._h)
        self._h = h
        self._comm = C.c_void_p(self._lib.tdx_rccl_comm_handle(h))
        self.backend = "rccl-native"
        del torch

    def ptr(self):
        return self._comm

    def _counters(self):
        e, a = C.c_int64(), C.c_int64()
        self._lib.tdx_rccl_comm_counters(self._h, C.byref(e), C.byref(a))
        return e.value, a.value

    @property
    def exchanges(self):
        return self._counters()[0]

    @property
    def allreduces(self):
        return self._counters()[1]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tdx_rccl_comm_destroy(self._h)
            self._h = None


class _GroupComm:
    """The tdx_comm of one rank of a StripGroup (owned by the group)."""

    def __init__(self, ptr, backend):
        self._ptr, self.backend = ptr, backend

    def ptr(self):
        return self._ptr


class StripGroup:
    """N row strips driven from ONE process: the library's own rank group (tdx_group_create, include/taudem_amd.h) - one context and
    one tdx_comm per rank; ranks that each have a device talk over RCCL, ranks that share a device over the in-process peer transport
    (host barriers + device copies).  `run(fn)` calls fn(rank, ctx, comm) on one thread per rank (the C calls release the GIL) and
    returns the results in rank order.  This is what `tool --gpus N` does in C++ (tool_strips.hpp); here it serves the tests and
    bench.py's functional many-strips-on-one-GPU runs."""

    def __init__(self, size: int, nx: int, devices=None):
        self._lib = _lib.load()
        self.size, self.nx = int(size), int(nx)
        devs = list(devices) if devices is not None else [0] * self.size
        arr = (C.c_int32 * self.size)(*devs)
        g = C.c_void_p()
        check(self._lib.tdx_group_create(self.size, arr, self.nx, C.byref(g)))
        self._g = g
        self.transport = self._lib.tdx_group_transport(g).decode()
        self.contexts = [api.Context.borrow(self._lib.tdx_group_context(g, r), devs[r]) for r in range(self.size)]
        self.comms = [_GroupComm(C.c_void_p(self._lib.tdx_group_comm(g, r)), self.transport) for r in range(self.size)]

    def run(self, fn):
        """fn(rank, context, comm) on one thread per rank; returns the list of results.  A rank that raises ABORTS THE GROUP (tdx_group_abort: the other
        ranks' pending and future collectives fail at once instead of waiting for TDX_COMM_TIMEOUT) - whatever it raised, communication error or
        not - and an aborted group is dead: its barrier and its RCCL communicators are gone for good.  run() on a dead group raises at once; build
        a new StripGroup to go on."""
        import threading

        if getattr(self, "_dead", False):
            raise RuntimeError("this StripGroup was aborted by a failed rank in an earlier run(): the rank group is one-shot after a failure - create a new StripGroup")
        out, err = [None] * self.size, []

        def main(r):
            try:
                out[r] = fn(r, self.contexts[r], self.comms[r])
            except BaseException as e:   # noqa: BLE001 - reported below
                import traceback
                err.append((r, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
                # the other ranks must not sit in their collectives until TDX_COMM_TIMEOUT: pending and future waits fail at once
                self._lib.tdx_group_abort(self._g)

        th = [threading.Thread(target=main, args=(r,), daemon=True) for r in range(self.size)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if err:
            self._dead = True
            raise RuntimeError("StripGroup rank(s) failed (the group is now dead - create a new one to continue):\n" + "\n".join(f"[rank {r}] {m}" for r, m in sorted(err)))
        return out

    def close(self):
        if getattr(self, "_g", None):
            for c in self.contexts:
                c.close()
            self._lib.tdx_group_destroy(self._g)
            self._g = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def project_critical_path(logs, exchange_us: float = 10.0, vote_us: float = 30.0, use: str = "wall"):
    """The critical path of an N-GPU strip run from the ranks' SEGMENT TRACES (Context.segments(), option "segment_trace" = 2: ranks that share a
    GPU take turns on it, so that every segment is timed as on a GPU of its own).  A strip run is, on every rank, the same sequence of
    segments of rank-local work separated by collectives (the outer loop of src/aread8.cpp:282-303 with share() / MPI_Allreduce,
    src/linearpart.h:313-384): a collective completes when the slowest rank arrives, so

        projected time = sum over segments of (max over ranks of the segment's time) + exchanges x exchange_us + all-reduces x vote_us.

    logs[r] = [(stage, phase, kind, device_ms, wall_ms), ...] of rank r.  Returns {"total_ms", "per_stage": {stage: {"ms", "work_ms", "latency_ms",
    "segments", "exchanges", "allreduces", "sum_over_ranks_ms", "phases": {phase: ms}}}, "assumed": {...}}.  A PROJECTION, not a measurement."""
    n = len(logs[0])
    for r, lg in enumerate(logs):
        if len(lg) != n or any(a[:3] != b[:3] for a, b in zip(lg, logs[0])):
            raise ValueError(f"rank {r} went through a different sequence of collectives than rank 0: the protocol is not rank-symmetric")
    col = 4 if use == "wall" else 3
    per, total = {}, 0.0
    for i in range(n):
        stage, phase, kind = logs[0][i][:3]
        work = max(lg[i][col] for lg in logs)
        lat = (exchange_us if kind == 0 else vote_us if kind == 1 else 0.0) * 1e-3
        st = per.setdefault(stage, {"ms": 0.0, "work_ms": 0.0, "latency_ms": 0.0, "segments": 0, "exchanges": 0, "allreduces": 0, "sum_over_ranks_ms": 0.0,
                                    "slowest_rank_histogram": [0] * len(logs), "phases": {}})
        st["ms"] += work + lat; st["work_ms"] += work; st["latency_ms"] += lat; st["segments"] += 1
        st["exchanges"] += kind == 0; st["allreduces"] += kind == 1
        st["sum_over_ranks_ms"] += sum(lg[i][col] for lg in logs)
        st["slowest_rank_histogram"][max(range(len(logs)), key=lambda r: logs[r][i][col])] += 1
        st["phases"][phase or "-"] = st["phases"].get(phase or "-", 0.0) + work + lat
        total += work + lat
    return {"total_ms": total, "per_stage": per,
            "assumed": {"exchange_us": exchange_us, "vote_us": vote_us, "segment_time": use,
                        "note": "projection from one-GPU segment traces (one rank on the device at a time), not an N-GPU measurement"}}


class _StripDropAnalysisStage:
    """StripPipeline.dropanalysis: a strip's partial counts and sums rather than rasters (include/taudem_amd_dropan.h)."""

    def dropanalysis(self, ad8, p, fel, ssa, outlets, thresh_min=5.0, thresh_max=500.0, nthresh=10, steptype=0, dx=1.0, dy=1.0, nodata=int(P_NODATA),
                     ssa_nodata=-1.0, grids=None):
        """thresh, n1, n2, sums, length, outlet_term = dropanalysis(ad8, p, fel, ssa, outlets) on this strip (src/DropAnalysis.cpp:172): the STRIP's own
        counts, fp64 sums and length per threshold and, per outlet, ad8 of the strip's terminal outlets (0 elsewhere).  Add the strips in strip
        order and the outlet terms in file order (times the cell area: the total area), then taudem_amd.dropanalysis_table makes the table and the
        optimum.  outlets: (columns, STRIP-ARRAY rows) as for aread8; the library fills the halo rows of p, fel and ssa."""
        return api._dropanalysis(self._call(), ad8, p, fel, ssa, outlets, thresh_min, thresh_max, nthresh, steptype, dx, dy, nodata, ssa_nodata, grids)


class _StripStreamNetStage:
    """StripPipeline.streamnet_compact / streamnet_label (include/taudem_amd_streamnet.h): the two strip halves of StreamNet.  Between them the parts
    of all strips meet in taudem_amd.api.StreamNetLinks (strip order = row-major order), which builds the links once on the host."""

    def streamnet_compact(self, p, src, fel, ad8, row0, dx=1.0, dy=1.0, nodata=int(P_NODATA), src_nodata=int(P_NODATA)):
        """part = streamnet_compact(p, src, fel, ad8, row0) on this strip: fills the halo rows of p and src (keep them for streamnet_label), runs the
        length sweep and returns the handle of the strip's stream cells.  row0: the global row of the strip's first owned row."""
        return api._streamnet_compact(self._call(), p, src, fel, ad8, row0, dx, dy, nodata, src_nodata)

    def streamnet_label(self, p, src, part, links, first_cell, single_watershed=False, nodata=int(P_NODATA), src_nodata=int(P_NODATA)):
        """ord, w = streamnet_label(p, src, part, links.handle, links.first_cell[rank]) on this strip: the owned rows are those of Context.streamnet."""
        return api._streamnet_label(self._call(), p, src, part, links, first_cell, single_watershed, nodata, src_nodata)


class _StripOutletToolsStage:
    """StripPipeline.moveoutletstostrm / connectdown_argmax / connectdown_walk (include/taudem_amd_outlets.h).  The walks advance the points that lie in
    this strip's owned rows and hand the state back: the caller passes it from strip to strip until a round over all strips moves nothing.  The
    maxima of all strips meet in taudem_amd.api.ConnectDownPoints (strip order = row-major order).  No halo row is read."""

    def moveoutletstostrm(self, p, src, row0, ny_total, state, maxdist=50, nodata=int(P_NODATA), src_nodata=int(P_NODATA)):
        """moved = moveoutletstostrm(p, src, row0, ny_total, state) on this strip: state = (columns, GLOBAL rows, dist, done), int32 numpy arrays advanced
        in place (start: dist 0, done 0); moved: the outlets this strip advanced or finished.  row0: the global row of the strip's first owned row."""
        return api._moveoutlets_strip(self._call(), p, src, row0, ny_total, maxdist, state, nodata, src_nodata)

    def connectdown_argmax(self, w, ad8, row0, w_nodata=-2147483647):
        """part = connectdown_argmax(w, ad8, row0) on this strip: the handle of the maxima of its owned rows, the table sized by the largest id of all strips."""
        return api._connectdown_strip(self._call(), w, ad8, row0, w_nodata)

    def connectdown_walk(self, p, w, row0, ny_total, state, movedist=10):
        """moved = connectdown_walk(p, w, row0, ny_total, state) on this strip: state = ConnectDownPoints.state(), advanced in place."""
        return api._connectdown_walk_strip(self._call(), p, w, row0, ny_total, movedist, state)


class _StripPeukerDouglasStage:
    """StripPipeline.peukerdouglas (include/taudem_amd_peuker.h)."""

    def peukerdouglas(self, fel, nodata=float(FEL_NODATA), weights=(0.4, 0.1, 0.05), float_weights=False, out=None):
        """ss = peukerdouglas(fel) on this strip (src/PeukerDouglas.cpp:54), or ss, w with float_weights: the two kernels with the smoothed grid between
        them.  The library fills the halo rows of fel and exchanges the smoothed edge rows; the halo rows of ss and w are not written."""
        return api._peukerdouglas(self._call(), fel, nodata, weights, float_weights, out)


class _StripSinmapStage:
    """StripPipeline.sinmapsi (include/taudem_amd_sinmap.h)."""

    def sinmapsi(self, slp, sca, cal, regions, rminter, rmaxter, g=9.81, rhow=1000.0, scamin=None, scamax=None, slp_nodata=float(api.SLOPE_NODATA), cal_nodata=-32768,
                 out=None):
        """si, sat = sinmapsi(slp, sca, cal, regions, rminter, rmaxter, g, rhow) on this strip (src/SinmapSI.cpp:138).  Cells are independent: the owned
        rows are computed, nothing is exchanged, and the halo rows of si and sat are not written."""
        return api._sinmapsi(self._call(), slp, sca, cal, regions, rminter, rmaxter, g, rhow, scamin, scamax, slp_nodata, cal_nodata, out)


class _StripTerrainIndexStage:
    """StripPipeline.terrain_indices, twi, slopearea, slopearearatio, lengtharea and setregion (include/taudem_amd_indices.h).  The first five exchange nothing;
    setregion fills the halo rows of p.  The halo rows of the outputs are not written."""

    def terrain_indices(self, slp, sca, m=2.0, n=1.0, want=api._lib.TERRAIN_OUTPUTS, slp_nodata=float(api.SLOPE_NODATA), sca_nodata=float(api.AREA_NODATA), out=None):
        """the outputs named in `want` (of "twi", "sa", "sar"), then the stats dict, on this strip."""
        return api._terrain_indices(self._call(), slp, sca, m, n, want, slp_nodata, sca_nodata, out)

    def twi(self, slp, sca, slp_nodata=float(api.SLOPE_NODATA), sca_nodata=float(api.AREA_NODATA), out=None):
        return api._terrain_indices(self._call(), slp, sca, 0.0, 0.0, ("twi",), slp_nodata, sca_nodata, None if out is None else (out,))

    def slopearea(self, slp, sca, m=2.0, n=1.0, out=None):
        return api._terrain_indices(self._call(), slp, sca, m, n, ("sa",), float(api.SLOPE_NODATA), float(api.AREA_NODATA), None if out is None else (out,))

    def slopearearatio(self, slp, sca, sca_nodata=float(api.AREA_NODATA), out=None):
        return api._terrain_indices(self._call(), slp, sca, 0.0, 0.0, ("sar",), float(api.SLOPE_NODATA), sca_nodata, None if out is None else (out,))

    def lengtharea(self, plen, ad8, M=0.03, y=1.3, out=None):
        """ss = lengtharea(plen, ad8) on this strip (src/LengthArea.cpp:51)."""
        return api._lengtharea(self._call(), plen, ad8, M, y, out)

    def setregion(self, p, gw, region_id=1, nodata=int(P_NODATA), gw_nodata=-2147483647, out=None):
        """region = setregion(p, gw, region_id) on this strip (src/SetRegion.cpp:78): the library fills the halo rows of p."""
        return api._setregion(self._call(), p, gw, region_id, nodata, gw_nodata, out)


class _StripEditRasterStage:
    """StripPipeline.editraster (include/taudem_amd_editraster.h): nothing is exchanged and the halo rows of the output are not written."""

    def editraster(self, raster, cols, rows, vals, row0, out=None, nodata=int(P_NODATA)):
        """new = editraster(raster, cols, rows, vals, row0) on this strip (src/EditRaster.cpp:69): rows are GLOBAL rows, row0 is the global row of the strip's
        first owned row; every strip is given the whole list and applies the changes of its owned rows.  out=raster edits the strip in place."""
        return api._editraster(self._call(), raster, cols, rows, vals, nodata, out, row0=row0)


class _StripPolygonizeStage:
    """StripPipeline.polygonize_edges (include/taudem_amd_polygonize.h).  Nothing is exchanged: the CALLER fills the halo rows of w with the neighbouring
    strips' rows; they are read and never written.  The parts of all strips meet in taudem_amd.api.Polygons (strip order = key order)."""

    def polygonize_edges(self, w, row0, ny_total, nodata=-2147483647):
        """part = polygonize_edges(w, row0, ny_total) on this strip: the handle of the boundary edges of its owned rows, with the keys of the whole raster.
        A halo row that lies outside rows 0 .. ny_total - 1 is off the raster whatever it holds."""
        return api._polygonize_edges_strip(self._call(), w, row0, ny_total, nodata)


class _StripRegionGridStage:
    """StripPipeline.regiongrid (include/taudem_amd_regions.h).  Nothing is exchanged and the halo rows of the output are left unwritten."""

    def regiongrid(self, gt, row0, ny_total, polygons=None, values=None, source=None, source_gt=None, source_nodata=-2147483647, out=None, workspace_words=0, phases=False):
        """grid, ids, stats = regiongrid(gt, row0, ny_total, ...) on this strip: its owned rows of the region grid of a raster of ny_total rows whose
        geotransform is gt, and the values that occur in them.  source: the WHOLE source grid as a tensor on this device.  phases=True: stats["phases"],
        at the price of a drained stream after every phase."""
        return api._regiongrid(self._call(), None, gt, polygons, values, source, source_gt, source_nodata, out, workspace_words, row0=row0, ny_total=ny_total, phases=phases)


class StripPipeline(_StripDropAnalysisStage, _StripPeukerDouglasStage, _StripStreamNetStage, _StripOutletToolsStage, _StripSinmapStage, _StripTerrainIndexStage,
                    _StripEditRasterStage, _StripPolygonizeStage, _StripRegionGridStage):
    """The tools of taudem_amd.api.Context on one strip of a row-partitioned raster.  All rasters are CUDA
    tensors of shape (ny_local + 2, nx): row 0 / row -1 are the halo rows the library maintains.  Every method
    runs the marshalling body of the Context method of its name (taudem_amd/api.py) on a strip frame, takes
    dx / dy as scalars or one value per row of the strip array (strip_rows()), and returns (outputs..., stats dict)."""

    def __init__(self, ctx, comm: StripComm | None, nx: int, ny_local: int):
        import torch

        self.ctx, self.comm, self.nx, self.ny_local = ctx, comm, int(nx), int(ny_local)
        self.torch = torch
        self.shape = (self.ny_local + 2, self.nx)
        self._cp = comm.ptr() if comm is not None else None

    def empty(self, dtype):
        return self.torch.empty(self.shape, dtype=dtype, device=f"cuda:{self.ctx.device}")

    def local_outlets(self, cols, global_rows, y0):
        """Global (column, row) outlet indices -> strip-array coordinates of the strip that starts at global row y0."""
        return np.asarray(cols, dtype=np.int32), (np.asarray(global_rows, dtype=np.int64) - int(y0) + 1).astype(np.int32)

    def _call(self):
        return api._Call(self.ctx, self.shape, self._cp)

    def pitremove(self, dem, nodata=-9999.0, fourway=False, out=None):
        return api._pitremove(self._call(), dem, nodata, None, fourway, out)

    def d8flowdir(self, fel, nodata=float(FEL_NODATA), dx=1.0, dy=1.0, out=None):
        return api._d8flowdir(self._call(), fel, nodata, dx, dy, True, out)

    def aread8(self, p, nodata=int(P_NODATA), weights=None, weights_nodata=-9999.0, contcheck=True, outlets=None, out=None):
        """outlets: (columns, STRIP-ARRAY rows) (local_outlets()); None = no outlets."""
        return api._aread8(self._call(), p, nodata, weights, weights_nodata, contcheck, outlets, out)

    def dinfflowdir(self, fel, nodata=float(FEL_NODATA), dx=1.0, dy=1.0, out=None):
        return api._dinfflowdir(self._call(), fel, nodata, dx, dy, out)

    def areadinf(self, ang, nodata=float(ANG_NODATA), dx=1.0, dy=1.0, weights=None, contcheck=True, outlets=None, out=None):
        return api._areadinf(self._call(), ang, nodata, dx, dy, weights, contcheck, outlets, out)

    def dinfupdependence(self, ang, dg, nodata=float(ANG_NODATA), dx=1.0, dy=1.0):
        """dep = depgrd(ang, dg) on this strip (src/DinfUpDependence.cpp:52): dg int32, dep float32 (nodata -1)."""
        return api._dinfupdependence(self._call(), ang, dg, nodata, dx, dy)

    def dinfrevaccum(self, ang, w, nodata=float(ANG_NODATA), w_nodata=-9999.0, dx=1.0, dy=1.0):
        """racc, dmax = dsaccum(ang, w) on this strip (src/DinfRevAccum.cpp:51)."""
        return api._dinfrevaccum(self._call(), ang, w, nodata, w_nodata, dx, dy)

    def dinfdistdown(self, ang, src, fel=None, *, stat="ave", kind="v", weights=None, weights_nodata=-9999.0, contcheck=True, dx=1.0, dy=1.0,
                     nodata=float(ANG_NODATA), fel_nodata=float(FEL_NODATA)):
        """dd = dinfdistdown(ang, fel, src, w) on this strip (src/DinfDistDown.cpp:66): src int16, dd float32 (nodata -FLT_MAX)."""
        return api._dinfdistdown(self._call(), ang, src, fel, stat, kind, weights, weights_nodata, contcheck, dx, dy, nodata, fel_nodata)

    def dinfdistup(self, ang, fel=None, *, stat="ave", kind="h", weights=None, weights_nodata=-9999.0, contcheck=True, thresh=0.0, dx=1.0, dy=1.0,
                   nodata=float(ANG_NODATA), fel_nodata=float(FEL_NODATA)):
        """du = dinfdistup(ang, fel, w) on this strip (src/DinfDistUp.cpp:65): du float32 (nodata -FLT_MAX)."""
        return api._dinfdistup(self._call(), ang, fel, stat, kind, weights, weights_nodata, contcheck, thresh, dx, dy, nodata, fel_nodata)

    def retlimflow(self, ang, wg, rc, *, dx=1.0, dy=1.0, nodata=float(ANG_NODATA), wg_nodata=-9999.0, rc_nodata=-9999.0):
        """qrl = retlimro(ang, wg, rc) on this strip (src/RetlimFlow.cpp:53): qrl float32 (nodata -FLT_MAX)."""
        return api._retlimflow(self._call(), ang, wg, rc, dx, dy, nodata, wg_nodata, rc_nodata)

    def dinfavalanche(self, ang, fel, ass, *, row0, ny_total, thresh=0.2, alpha=18.0, direct=False, dx=1.0, dy=1.0, geo=None, geographic=False,
                      nodata=float(ANG_NODATA), fel_nodata=float(FEL_NODATA), ass_nodata=-32768):
        """rz, dfs = avalancherunoutgrd(ang, fel, ass) on this strip (src/DinfAvalanche.cpp:62).  row0: global row of the strip's first owned row,
        ny_total: rows of the whole raster; geo = (xleftedge, ytopedge, dlon, dlat) of the WHOLE raster (direct mode)."""
        return api._dinfavalanche(self._call(), ang, fel, ass, thresh, alpha, direct, dx, dy, geo, geographic, nodata, fel_nodata, ass_nodata,
                                  whole=(int(row0), int(ny_total)))

    def d8hdisttostrm(self, p, src, thresh=1, *, dx=1.0, dy=1.0, nodata=int(P_NODATA), src_nodata=-2147483647):
        """dist = distgrid(p, src) on this strip (src/D8HDistToStrm.cpp:57): src int32, dist float32 (nodata -FLT_MAX)."""
        return api._d8hdisttostrm(self._call(), p, src, thresh, dx, dy, nodata, src_nodata)

    def d8vdisttostrm(self, p, fel, src, thresh=1, *, nodata=int(P_NODATA), src_nodata=-2147483647):
        """dist = d8vdistdown(p, fel, src) on this strip (src/D8VDistToStrm.cpp:58).  fel's halo rows are exchanged (written) by the call."""
        return api._d8vdisttostrm(self._call(), p, fel, src, thresh, nodata, src_nodata)

    def flowdircond(self, p, z, *, nodata=int(P_NODATA), z_nodata=float(FEL_NODATA)):
        """zfdc = flowdircond(p, z) on this strip (src/flowdircond.cpp:54)."""
        return api._flowdircond(self._call(), p, z, nodata, z_nodata)

    def slopeavedown(self, p, fel, dn, niter, *, dx=1.0, dy=1.0, nodata=int(P_NODATA), fel_nodata=float(FEL_NODATA)):
        """slpd = sloped(p, fel, dn) on this strip (src/SlopeAveDown.cpp:59).  niter: the pass count of the WHOLE raster
        (int(dn / min(dx, dy) of its middle row) + 1); the record halo rows are exchanged after every pass."""
        return api._slopeavedown(self._call(), p, fel, dn, int(niter), dx, dy, nodata, fel_nodata)

    def gagewatershed(self, p, outlets, *, nodata=int(P_NODATA)):
        """gw, id_table = gagewatershed(p, outlets) on this strip (src/gagewatershed.cpp:56).  outlets: (columns, STRIP-ARRAY rows, ids) of ALL
        outlets (local_outlets(); those outside the owned rows are other ranks'); id_table as Context.gagewatershed's, the same on every rank."""
        return api._gagewatershed(self._call(), p, outlets[0], outlets[1], outlets[2], nodata)

    def dinfdecayaccum(self, ang, dm, nodata=float(ANG_NODATA), dm_nodata=-9999.0, dx=1.0, dy=1.0, weights=None, contcheck=True, outlets=None, out=None):
        return api._dinfdecayaccum(self._call(), ang, dm, nodata, dm_nodata, dx, dy, weights, contcheck, outlets, out)

    def d8flowpathextremeup(self, p, sa, nodata=int(P_NODATA), usemax=True, contcheck=True, outlets=None):
        """ssa = d8flowpathextremeup(p, sa) on this strip (src/D8flowpathextremeup.cpp:58): sa float32, ssa float32 (nodata -FLT_MAX).
        outlets: (columns, STRIP-ARRAY rows) as for aread8."""
        return api._d8flowpathextremeup(self._call(), p, sa, nodata, usemax, contcheck, outlets, None)

    def gridnet(self, p, nodata=int(P_NODATA), dx=1.0, dy=1.0, mask=None, thresh=0, outlets=None):
        """plen, tlen, gord = gridnet(p) on this strip (src/gridnet.cpp:54): mask an optional int32 strip array (the library fills its halo
        rows); outlets: (columns, STRIP-ARRAY rows) as for aread8."""
        return api._gridnet(self._call(), p, nodata, dx, dy, mask, thresh, outlets)

    def dinfconclimaccum(self, ang, dm, dg, q, csol=1.0, nodata=float(ANG_NODATA), dm_nodata=-9999.0, q_nodata=-9999.0, dx=1.0, dy=1.0, contcheck=True,
                         outlets=None):
        """ctpt = dsllArea(ang, dm, dg, q) on this strip (src/DinfConcLimAccum.cpp:61): dg int16, ctpt float32 (nodata -FLT_MAX)."""
        return api._dinfconclimaccum(self._call(), ang, dm, dg, q, csol, nodata, dm_nodata, q_nodata, dx, dy, contcheck, outlets)

    def dinftranslimaccum(self, ang, tsup, tc, cs=None, nodata=float(ANG_NODATA), tsup_nodata=-9999.0, tc_nodata=-9999.0, cs_nodata=-9999.0, dx=1.0, dy=1.0,
                          contcheck=True, outlets=None):
        """tla, tdep, ctpt = tlaccum(ang, tsup, tc[, cs]) on this strip (src/DinfTransLimAccum.cpp:61): float32, nodata -FLT_MAX; ctpt is None
        without cs."""
        return api._dinftranslimaccum(self._call(), ang, tsup, tc, cs, nodata, tsup_nodata, tc_nodata, cs_nodata, dx, dy, contcheck, outlets)
