"""ctypes binding of libtaudem_amd.so (the C ABI declared in include/taudem_amd.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C taudem_amd/csrc``.  There is
no CPU fallback: if the library is missing the import fails loudly, and compute entry points fail
with ``TDX_ERR_NOGPU`` when no HIP device is present.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtaudem_amd.so")

TDX_OK = 0
TDX_ERR_MISMATCH = 1
TDX_ERR_OUTLETS = 5
TDX_ERR_FILE = 21
TDX_ERR_DRIVER = 22
TDX_ERR_ARG = -1
TDX_ERR_HIP = -2
TDX_ERR_NOGPU = -3
TDX_ERR_NOMEM = -999

TDX_DT_I16, TDX_DT_I32, TDX_DT_F32 = 0, 1, 2

K_STENCIL, K_RELAX, K_BFS, K_FLATDIR, K_ACCUM, K_MISC, K_TILEK = 0, 1, 2, 3, 4, 5, 6
KERNEL_CLASSES = {"stencil": K_STENCIL, "relax": K_RELAX, "bfs": K_BFS, "flatdir": K_FLATDIR, "accum": K_ACCUM, "misc": K_MISC, "tilek": K_TILEK}


class TdxStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_double),
        ("ms_kernel", C.c_double * 8),
        ("launches", C.c_int64 * 8),
        ("rounds", C.c_int64),
        ("flats_initial", C.c_int64),
        ("flats_left", C.c_int64),
        ("flat_iterations", C.c_int64),
        ("levels_fall", C.c_int64),
        ("levels_rise", C.c_int64),
        ("cells_evaluated", C.c_int64),
        ("levels_fall_max", C.c_int64),
        ("levels_rise_max", C.c_int64),
    ]

    def as_dict(self):
        d = {
            "ms_total": self.ms_total,
            "rounds": self.rounds,
            "flats_initial": self.flats_initial,
            "flats_left": self.flats_left,
            "flat_iterations": self.flat_iterations,
            "levels_fall": self.levels_fall,
            "levels_rise": self.levels_rise,
            "cells_evaluated": self.cells_evaluated,
            "levels_fall_max": self.levels_fall_max,
            "levels_rise_max": self.levels_rise_max,
        }
        for name, k in KERNEL_CLASSES.items():
            d["ms_" + name] = self.ms_kernel[k]
            d["launches_" + name] = self.launches[k]
        return d


class TdxSegment(C.Structure):
    """struct tdx_segment of include/taudem_amd.h (segment trace of a strip run)."""
    _fields_ = [("stage", C.c_char * 24), ("phase", C.c_char * 24), ("kind", C.c_int32), ("device_ms", C.c_float), ("wall_ms", C.c_float)]


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32)


class TdxComm(C.Structure):
    """struct tdx_comm of include/taudem_amd.h (row strips across GPUs)."""
    _fields_ = [
        ("rank", C.c_int32),
        ("size", C.c_int32),
        ("user", C.c_void_p),
        ("exchange", EXCHANGE_FN),
        ("allreduce", ALLREDUCE_FN),
        ("send_up", C.c_void_p),
        ("send_down", C.c_void_p),
        ("recv_up", C.c_void_p),
        ("recv_down", C.c_void_p),
        ("capacity", C.c_uint64),
        ("flags", C.c_uint64),              # 0: host-synchronous contract (this Python transport)
        ("allreduce_dev", C.c_void_p),      # NULL: votes travel through `allreduce` on host values
    ]


class TdxRasterInfo(C.Structure):
    _fields_ = [
        ("nx", C.c_int64),
        ("ny", C.c_int64),
        ("geotransform", C.c_double * 6),
        ("nodata", C.c_double),
        ("has_nodata", C.c_int32),
        ("geographic", C.c_int32),
        ("dxA", C.c_double),
        ("dyA", C.c_double),
    ]


_P = C.c_void_p
_I64 = C.c_int64
_F = C.c_float
_INT, _I16, _I32, _D = C.c_int, C.c_int16, C.c_int32, C.c_double

# tool -> argtypes of tdx_<tool>, under the argument names of include/taudem_amd.h.  tdx_<tool>_dev takes the same list with device rasters,
# tdx_<tool>_strip the comm pointer after the context (and ny_local for ny): _signatures() writes the three rows out.
_TOOLS = {
    # ctx, dem, nx, ny, dem_nodata, mask, fourway, fel, stats
    "pitremove": [_P, _P, _I64, _I64, _F, _P, _INT, _P, _P],
    # ctx, fel, nx, ny, fel_nodata, dxc, dyc, p, sd8, stats
    "d8flowdir": [_P, _P, _I64, _I64, _F, _P, _P, _P, _P, _P],
    # ctx, p, nx, ny, p_nodata, w, w_nodata, contcheck, outlet_x, outlet_y, n_outlets, ad8, stats
    "aread8": [_P, _P, _I64, _I64, _I16, _P, _F, _INT, _P, _P, _I64, _P, _P],
    # ctx, p, nx, ny, p_nodata, sa, usemax, contcheck, outlet_x, outlet_y, n_outlets, ssa, stats
    "d8flowpathextremeup": [_P, _P, _I64, _I64, _I16, _P, _INT, _INT, _P, _P, _I64, _P, _P],
    # ctx, p, nx, ny, p_nodata, dxc, dyc, mask, thresh, outlet_x, outlet_y, n_outlets, plen, tlen, gord, stats
    "gridnet": [_P, _P, _I64, _I64, _I16, _P, _P, _P, _I32, _P, _P, _I64, _P, _P, _P, _P],
    # ctx, ssa, nx, ny, ssa_nodata, mask, thresh, src, stats (no strip form)
    "threshold": [_P, _P, _I64, _I64, _F, _P, _F, _P, _P],
    # ctx, fel, nx, ny, fel_nodata, dxc, dyc, ang, slp, stats
    "dinfflowdir": [_P, _P, _I64, _I64, _F, _P, _P, _P, _P, _P],
    # ctx, ang, nx, ny, ang_nodata, dxc, dyc, w, contcheck, outlet_x, outlet_y, n_outlets, sca, stats
    "areadinf": [_P, _P, _I64, _I64, _F, _P, _P, _P, _INT, _P, _P, _I64, _P, _P],
    # ctx, ang, nx, ny, ang_nodata, dxc, dyc, dm, dm_nodata, w, contcheck, outlet_x, outlet_y, n_outlets, dsca, stats
    "dinfdecayaccum": [_P, _P, _I64, _I64, _F, _P, _P, _P, _F, _P, _INT, _P, _P, _I64, _P, _P],
    # ctx, ang, nx, ny, ang_nodata, dxc, dyc, dg, dep, stats
    "dinfupdependence": [_P, _P, _I64, _I64, _F, _P, _P, _P, _P, _P],
    # ctx, ang, nx, ny, ang_nodata, dxc, dyc, w, w_nodata, racc, dmax, stats
    "dinfrevaccum": [_P, _P, _I64, _I64, _F, _P, _P, _P, _F, _P, _P, _P],
    # ctx, ang, nx, ny, ang_nodata, dxc, dyc, fel, fel_nodata, src, w, w_nodata, statmethod, typemethod, contcheck, dd, stats
    "dinfdistdown": [_P, _P, _I64, _I64, _F, _P, _P, _P, _F, _P, _P, _F, _INT, _INT, _INT, _P, _P],
    # ctx, ang, nx, ny, ang_nodata, dxc, dyc, fel, fel_nodata, w, w_nodata, statmethod, typemethod, contcheck, thresh, du, stats
    "dinfdistup": [_P, _P, _I64, _I64, _F, _P, _P, _P, _F, _P, _F, _INT, _INT, _INT, _F, _P, _P],
    # ctx, p, nx, ny, p_nodata, src, src_nodata, thresh, dxc, dyc, dist, stats
    "d8hdisttostrm": [_P, _P, _I64, _I64, _I16, _P, _I32, _I32, _P, _P, _P, _P],
    # ctx, p, nx, ny, p_nodata, outlet_x, outlet_y, ids, n_outlets, gw, placed, iddown, stats
    "gagewatershed": [_P, _P, _I64, _I64, _I16, _P, _P, _P, _I64, _P, _P, _P, _P],
    # ctx, p, nx, ny, p_nodata, fel, src, src_nodata, thresh, dist, stats
    "d8vdisttostrm": [_P, _P, _I64, _I64, _I16, _P, _P, _I32, _I32, _P, _P],
    # ctx, p, nx, ny, p_nodata, z, z_nodata, zfdc, stats
    "flowdircond": [_P, _P, _I64, _I64, _I16, _P, _F, _P, _P],
    # ctx, p, nx, ny, p_nodata, fel, fel_nodata, dxc, dyc, dn, niter, slpd, stats
    "slopeavedown": [_P, _P, _I64, _I64, _I16, _P, _F, _P, _P, _D, _I64, _P, _P],
    # ctx, hand, catch, slp, nx, ny, hand_nodata, catch_nodata, slp_nodata, dxc, dyc, ids, ncatch, stages, nheight, count, surface, bed, volume,
    # catcharea, stats
    "catchhydrogeo": [_P, _P, _P, _P, _I64, _I64, _F, _I32, _F, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P],
    # ctx, hand, catch, mask, nx, ny, hand_nodata, catch_nodata, mask_nodata, dxc, dyc, ids, depth, nfc, map, area, stats
    "inundepth": [_P, _P, _P, _P, _I64, _I64, _F, _I32, _I16, _P, _P, _P, _P, _I64, _P, _P, _P],
    # ctx, ang, nx, ny, ang_nodata, dxc, dyc, wg, wg_nodata, rc, rc_nodata, qrl, stats
    "retlimflow": [_P, _P, _I64, _I64, _F, _P, _P, _P, _F, _P, _F, _P, _P],
    # ctx, ang, nx, ny, ang_nodata, dxc, dyc, fel, fel_nodata, ass, ass_nodata, thresh, alpha, path, geo, geographic, rz, dfs, stats
    "dinfavalanche": [_P, _P, _I64, _I64, _F, _P, _P, _P, _F, _P, _I16, _F, _F, _INT, _P, _INT, _P, _P, _P],
    # ctx, ang, nx, ny, ang_nodata, dxc, dyc, dm, dm_nodata, dg, q, q_nodata, csol, contcheck, outlet_x, outlet_y, n_outlets, ctpt, stats
    "dinfconclimaccum": [_P, _P, _I64, _I64, _F, _P, _P, _P, _F, _P, _P, _F, _F, _INT, _P, _P, _I64, _P, _P],
    # ctx, ang, nx, ny, ang_nodata, dxc, dyc, tsup, tsup_nodata, tc, tc_nodata, cs, cs_nodata, contcheck, outlet_x, outlet_y, n_outlets, tla, tdep,
    # ctpt, stats
    "dinftranslimaccum": [_P, _P, _I64, _I64, _F, _P, _P, _P, _F, _P, _F, _P, _F, _INT, _P, _P, _I64, _P, _P, _P, _P],
}


def _signatures():
    """tdx_<tool>, tdx_<tool>_dev and tdx_<tool>_strip of every tool in _TOOLS."""
    out = {}
    for tool, args in _TOOLS.items():
        out["tdx_" + tool] = out["tdx_" + tool + "_dev"] = (C.c_int, args)
        if tool != "threshold":
            out["tdx_" + tool + "_strip"] = (C.c_int, args[:1] + [_P] + args[1:])
    # ..., geographic, row0, ny_total, rz, dfs, stats: the strip says where it lies in the whole raster
    out["tdx_dinfavalanche_strip"] = (C.c_int, out["tdx_dinfavalanche_strip"][1][:-3] + [_I64, _I64, _P, _P, _P])
    return out


# name -> (restype, argtypes): every symbol include/taudem_amd.h declares
_SIGNATURES = {
    **_signatures(),
    "tdx_context_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "tdx_context_destroy": (None, [_P]),
    "tdx_context_release_scratch": (C.c_int, [_P]),
    "tdx_last_error": (C.c_char_p, [_P]),
    "tdx_synchronize": (C.c_int, [_P]),
    "tdx_stream": (_P, [_P]),
    "tdx_version": (C.c_char_p, []),
    "tdx_context_set_option": (C.c_int, [_P, C.c_char_p, _I64]),
    "tdx_device_count": (C.c_int, []),
    "tdx_device_alloc": (C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    "tdx_device_free": (C.c_int, [_P, _P]),
    "tdx_copy_to_device": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "tdx_copy_to_host": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "tdx_tool_dinfdistdown": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tdx_tool_d8hdisttostrm": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    "tdx_tool_gagewatershed": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p]),
    "tdx_tool_d8vdisttostrm": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    "tdx_tool_flowdircond": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p]),
    "tdx_slopeavedown_niter": (_I64, [C.c_double, _P, _P, _I64]),
    "tdx_tool_slopeavedown": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_double]),
    "tdx_tool_catchhydrogeo": (C.c_int, [C.c_char_p] * 6),
    "tdx_tool_inundepth": (C.c_int, [C.c_char_p] * 7),
    "tdx_tool_dinfdistup": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, _F]),
    "tdx_tool_retlimflow": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
    "tdx_tool_dinfavalanche": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, _F, _F, C.c_int]),
    "tdx_tool_dinfupdependence": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p]),
    "tdx_tool_dinfrevaccum": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
    "tdx_tool_dinfconclimaccum": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_float]),
    "tdx_tool_dinftranslimaccum": (C.c_int, [C.c_char_p] * 9 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tdx_synth_dem_dev": (C.c_int, [_P, C.c_uint64, _I64, _I64, _I64, _I64, _I64, _P]),
    "tdx_raster_info_read": (C.c_int, [C.c_char_p, C.POINTER(TdxRasterInfo)]),
    "tdx_raster_read": (C.c_int, [C.c_char_p, C.c_int, _P, _P, _P]),
    "tdx_raster_write": (C.c_int, [C.c_char_p, C.c_int, _P, _I64, _I64, C.c_double, C.c_char_p, C.c_int]),
    "tdx_raster_write_geo": (C.c_int, [C.c_char_p, C.c_int, _P, _I64, _I64, C.c_double, _P, C.c_int, C.c_int]),
    "tdx_tool_pitremove": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]),
    "tdx_tool_d8flowdir": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    "tdx_tool_aread8": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int]),
    "tdx_tool_dinfflowdir": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    "tdx_tool_areadinf": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int]),
    "tdx_tool_dinfdecayaccum": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int]),
    "tdx_tool_gridnet": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tdx_tool_d8flowpathextremeup": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tdx_tool_threshold": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_float, C.c_int]),
    "tdx_outlets_read": (C.c_int, [C.c_char_p, _P, _P, _P, _I64, C.POINTER(_I64)]),
    "tdx_outlets_to_cells": (C.c_int, [C.c_char_p, _P, _P, _I64, _P, _P]),
    "tdx_tool_set_device": (C.c_int, [C.c_int]),
    "tdx_tool_set_gpus": (C.c_int, [C.c_int]),
    "tdx_rccl_unique_id": (C.c_int, [_P]),
    "tdx_rccl_comm_create": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _I64, C.POINTER(_P)]),
    "tdx_rccl_comm_handle": (_P, [_P]),
    "tdx_rccl_comm_counters": (None, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "tdx_rccl_comm_destroy": (None, [_P]),
    "tdx_rccl_selftest": (C.c_int, [_P]),
    "tdx_comm_latency": (C.c_int, [_P, _P, C.c_int32, C.c_uint64, C.POINTER(C.c_double)]),
    "tdx_rccl_latency": (C.c_int, [_P, C.c_int32, C.c_uint64, C.POINTER(C.c_double)]),
    "tdx_context_comm_counters": (None, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tdx_context_segments": (_I64, [_P, C.POINTER(TdxSegment), _I64]),
    "tdx_group_create": (C.c_int, [C.c_int32, _P, _I64, C.POINTER(_P)]),
    "tdx_group_context": (_P, [_P, C.c_int32]),
    "tdx_group_comm": (_P, [_P, C.c_int32]),
    "tdx_group_transport": (C.c_char_p, [_P]),
    "tdx_group_abort": (None, [_P]),
    "tdx_group_destroy": (None, [_P]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# name -> (restype, argtypes): the symbols include/taudem_amd_dropan.h declares, the extension header that taudem_amd.h includes
_DROPAN_SIGNATURES = {
    # DropAnalysis: ctx, ad8, p, fel, ssa, nx, ny, p_nodata, ssa_nodata, dxc, dyc, dxA, dyA, outlet_x, outlet_y, n_outlets, thresh_min, thresh_max, nthresh, steptype,
    # grid_th, order, elevout, thresh, n1, n2, sums, length, total_area, optimum, found, table, table_cap, stats.  The strip form has the comm after the context, no dxA / dyA,
    # and outlet_term in the place of total_area ... table_cap.
    "tdx_dropanalysis": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _I16, _F, _P, _P, _D, _D, _P, _P, _I64, _F, _F, _I64, _INT, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "tdx_dropanalysis_dev": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _I16, _F, _P, _P, _D, _D, _P, _P, _I64, _F, _F, _I64, _INT, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "tdx_dropanalysis_strip": (C.c_int, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I16, _F, _P, _P, _P, _P, _I64, _F, _F, _I64, _INT, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    # nthresh, thresh, n1, n2, s1, s1sq, s2, s2sq, length, total_area, table, table_cap, console, console_cap, optimum, found
    "tdx_dropanalysis_table": (C.c_int, [_I64, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _I64, _P, _I64, _P, _P]),
    "tdx_tool_dropanalysis": (C.c_int, [C.c_char_p] * 7 + [C.c_int, C.c_int, _F, _F, C.c_int, C.c_int, _P]),
}
DROPAN_SYMBOLS = tuple(_DROPAN_SIGNATURES)

# name -> (restype, argtypes): the symbols include/taudem_amd_peuker.h declares, the second extension header
_PEUKER_SIGNATURES = {
    # PeukerDouglas: ctx, fel, nx, ny, fel_nodata, w_center, w_side, w_diag, ss, w (optional), stats; the strip form has the comm after the context
    "tdx_peukerdouglas": (C.c_int, [_P, _P, _I64, _I64, _F, _F, _F, _F, _P, _P, _P]),
    "tdx_peukerdouglas_dev": (C.c_int, [_P, _P, _I64, _I64, _F, _F, _F, _F, _P, _P, _P]),
    "tdx_peukerdouglas_strip": (C.c_int, [_P, _P, _P, _I64, _I64, _F, _F, _F, _F, _P, _P, _P]),
    "tdx_tool_peukerdouglas": (C.c_int, [C.c_char_p, C.c_char_p, _P]),
}
PEUKER_SYMBOLS = tuple(_PEUKER_SIGNATURES)

# name -> (restype, argtypes): the symbol include/taudem_amd_ad8.h declares, the third extension header
_AD8_SIGNATURES = {
    "tdx_context_ad8_tile_counters": (None, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}
AD8_SYMBOLS = tuple(_AD8_SIGNATURES)

# name -> (restype, argtypes): the symbols include/taudem_amd_streamnet.h declares, the fourth extension header
_STREAMNET_HEAD = [_P, _P, _P, _P, _P, _I64, _I64, _I16, C.c_int32, _P, _P, _D, _D, _P, _P, _P, _P, _I64, _INT, _P, _P, C.POINTER(_P), _P]
_STREAMNET_SIGNATURES = {
    # StreamNet: ctx, p, src, fel, ad8, nx, ny, p_nodata, src_nodata, dxc, dyc, dxA, dyA, gt, outlet_x, outlet_y, outlet_id, n_outlets, single_watershed, ord, w,
    # &links, stats
    "tdx_streamnet": (C.c_int, _STREAMNET_HEAD),
    "tdx_streamnet_dev": (C.c_int, _STREAMNET_HEAD),
    # the same with the links built on the device (streamnet_links_device.hip)
    "tdx_streamnet_gpu_links": (C.c_int, _STREAMNET_HEAD),
    "tdx_streamnet_gpu_links_dev": (C.c_int, _STREAMNET_HEAD),
    # links, ms [STREAMNET_LINK_PHASES], jump_rounds, level_rounds, workspace_bytes -> 1 when the device built the links
    "tdx_streamnet_links_device_phases": (C.c_int, [_P, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64)]),
    "tdx_streamnet_links_count": (_I64, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "tdx_streamnet_links_copy": (None, [_P, _P, _P, _P]),
    "tdx_streamnet_links_free": (None, [_P]),
    # strips: ctx, comm, p, src, fel, ad8, nx, ny_local, row0, p_nodata, src_nodata, dxc, dyc, &part, stats
    "tdx_streamnet_compact_strip": (C.c_int, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I16, C.c_int32, _P, _P, C.POINTER(_P), _P]),
    "tdx_streamnet_compact_count": (_I64, [_P]),
    "tdx_streamnet_compact_free": (None, [_P]),
    # parts, n_parts, nx, ny, dxA, dyA, gt, outlet_x, outlet_y, outlet_id, n_outlets, &links
    "tdx_streamnet_links_build": (C.c_int, [_P, _I64, _I64, _I64, _D, _D, _P, _P, _P, _P, _I64, C.POINTER(_P)]),
    # ctx, comm, p, src, nx, ny_local, p_nodata, src_nodata, part, links, first_cell, single_watershed, ord, w, stats
    # ctx, then the arguments of tdx_streamnet_links_build
    "tdx_streamnet_links_build_gpu": (C.c_int, [_P, _P, _I64, _I64, _I64, _D, _D, _P, _P, _P, _P, _I64, C.POINTER(_P)]),
    "tdx_streamnet_label_strip": (C.c_int, [_P, _P, _P, _P, _I64, _I64, _I16, C.c_int32, _P, _P, _I64, _INT, _P, _P, _P]),
    "tdx_streamnet_write_text": (C.c_int, [_P, C.c_char_p, C.c_char_p]),
    "tdx_streamnet_net_rows": (C.c_int, [_P, _P, _I64, _I64, C.c_int, _I64, _P, _P, _P, _P]),
    "tdx_streamnet_net_write": (C.c_int, [_P, C.c_int, C.c_char_p]),
    "tdx_tool_streamnet": (C.c_int, [C.c_char_p] * 9 + [C.c_int, C.c_int] + [C.c_char_p] * 3 + [C.c_long, C.c_long, C.c_int]),
    "tdx_tool_set_streamnet_links": (C.c_int, [C.c_int]),
}
STREAMNET_SYMBOLS = tuple(_STREAMNET_SIGNATURES)
STREAMNET_PHASES = ("setup", "length", "compact", "links", "scatter", "label", "total")
STREAMNET_LINKS = ("host", "device")   # where the links are built: the value of tdx_tool_set_streamnet_links is the index
STREAMNET_LINK_PHASES = ("classify", "jump", "level", "number", "links", "rows", "download")   # the device builder's sub-phases

# name -> (restype, argtypes): the symbols include/taudem_amd_outlets.h declares, the fifth extension header
# MoveOutletsToStrm: ctx, p, src, nx, ny, p_nodata, src_nodata, maxdist, outlet_x, outlet_y, n_outlets, out_x, out_y, dist_moved, stats
_MOVEOUTLETS_HEAD = [_P, _P, _P, _I64, _I64, _I16, _I32, _I32, _P, _P, _I64, _P, _P, _P, _P]
# ConnectDown: ctx, p, w, ad8, nx, ny, p_nodata, w_nodata, movedist, &points, stats
_CONNECTDOWN_HEAD = [_P, _P, _P, _P, _I64, _I64, _I16, _I32, _I32, C.POINTER(_P), _P]
_OUTLETS_SIGNATURES = {
    "tdx_moveoutlets": (C.c_int, _MOVEOUTLETS_HEAD),
    "tdx_moveoutlets_dev": (C.c_int, _MOVEOUTLETS_HEAD),
    # ctx, comm, p, src, nx, ny_local, row0, ny_total, p_nodata, src_nodata, maxdist, state_x, state_y, state_dist, state_done, n_outlets, &n_moved, stats
    "tdx_moveoutlets_strip": (C.c_int, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _I16, _I32, _I32, _P, _P, _P, _P, _I64, C.POINTER(_I64), _P]),
    "tdx_connectdown": (C.c_int, _CONNECTDOWN_HEAD),
    "tdx_connectdown_dev": (C.c_int, _CONNECTDOWN_HEAD),
    "tdx_connectdown_points_count": (_I64, [_P]),
    # points, ids, x, y, ad8max, moved_x, moved_y, id_down, phase_ms
    "tdx_connectdown_points_copy": (None, [_P] * 9),
    "tdx_connectdown_points_free": (None, [_P]),
    # ctx, comm, w, ad8, nx, ny_local, row0, w_nodata, &part, stats
    "tdx_connectdown_strip": (C.c_int, [_P, _P, _P, _P, _I64, _I64, _I64, _I32, C.POINTER(_P), _P]),
    "tdx_connectdown_merge": (C.c_int, [_P, _I64, C.POINTER(_P)]),
    # ctx, comm, p, w, nx, ny_local, row0, ny_total, movedist, state_x, state_y, state_dist, state_done, id_down, n_points, &n_moved, stats
    "tdx_connectdown_walk_strip": (C.c_int, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _I32, _P, _P, _P, _P, _P, _I64, C.POINTER(_I64), _P]),
    "tdx_connectdown_points_set_moved": (C.c_int, [_P, _P, _P, _P]),
    # path, x, y, n, nfields, names, types, columns
    "tdx_points_write": (C.c_int, [C.c_char_p, _P, _P, _I64, _I32, _P, _P, _P]),
    "tdx_tool_moveoutletstostrm": (C.c_int, [C.c_char_p] * 4 + [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int]),
    "tdx_tool_connectdown": (C.c_int, [C.c_char_p] * 7 + [C.c_int]),
}
OUTLETS_SYMBOLS = tuple(_OUTLETS_SIGNATURES)
CONNECTDOWN_PHASES = ("maxid", "argmax", "decode", "walk")
CONNECTDOWN_MAX_ID = 134217727   # TDX_CONNECTDOWN_MAX_ID

# name -> (restype, argtypes): the symbols include/taudem_amd_sinmap.h declares, the sixth extension header
# SinmapSI: ctx, slp, sca, scamin, scamax (both optional), cal, nx, ny, slp_nodata, cal_nodata, nreg, reg_id, tmin, tmax, cmin, cmax, phimin, phimax, rhos,
# rminter, rmaxter, g, rhow, si, sat, stats; the strip form has the comm after the context
_SINMAP_TAIL = [_P, _P, _P, _P, _P, _I64, _I64, _F, C.c_double, _I32] + [_P] * 8 + [C.c_double, C.c_double, _F, _F, _P, _P, _P]
_SINMAP_SIGNATURES = {
    "tdx_sinmapsi": (C.c_int, [_P] + _SINMAP_TAIL),
    "tdx_sinmapsi_dev": (C.c_int, [_P] + _SINMAP_TAIL),
    "tdx_sinmapsi_strip": (C.c_int, [_P, _P] + _SINMAP_TAIL),
    # path, capacity, reg_id, tmin, tmax, cmin, cmax, phimin, phimax, rhos, &count
    "tdx_sinmap_read_calpar": (C.c_int, [C.c_char_p, _I32] + [_P] * 8 + [C.POINTER(_I32)]),
    # slp, sca, scamin, scamax, cal, calpar, sat, si, rminter, rmaxter, par
    "tdx_tool_sinmapsi": (C.c_int, [C.c_char_p] * 8 + [C.c_double, C.c_double, _P]),
}
SINMAP_SYMBOLS = tuple(_SINMAP_SIGNATURES)
SINMAP_FIELDS = ("id", "tmin", "tmax", "cmin", "cmax", "phimin", "phimax", "rhos")   # the columns of a -calpar file

# name -> (restype, argtypes): the symbols include/taudem_amd_indices.h declares, the seventh extension header
# terrain indices: ctx, slp, sca, nx, ny, slp_nodata, sca_nodata, m, n, twi, sa, sar (each optional, not all three), stats
_TERRAIN_TAIL = [_P, _P, _I64, _I64, _F, _F, _F, _F, _P, _P, _P, _P]
# LengthArea: ctx, plen, ad8, nx, ny, M, y, ss, stats
_LENGTHAREA_TAIL = [_P, _P, _I64, _I64, _F, _F, _P, _P]
# SetRegion: ctx, p, gw, nx, ny, p_nodata, gw_nodata, region_id, out, stats
_SETREGION_TAIL = [_P, _P, _I64, _I64, _I16, _I32, _I32, _P, _P]
_INDICES_SIGNATURES = {
    "tdx_terrain_indices": (C.c_int, [_P] + _TERRAIN_TAIL),
    "tdx_terrain_indices_dev": (C.c_int, [_P] + _TERRAIN_TAIL),
    "tdx_terrain_indices_strip": (C.c_int, [_P, _P] + _TERRAIN_TAIL),
    "tdx_lengtharea": (C.c_int, [_P] + _LENGTHAREA_TAIL),
    "tdx_lengtharea_dev": (C.c_int, [_P] + _LENGTHAREA_TAIL),
    "tdx_lengtharea_strip": (C.c_int, [_P, _P] + _LENGTHAREA_TAIL),
    "tdx_setregion": (C.c_int, [_P] + _SETREGION_TAIL),
    "tdx_setregion_dev": (C.c_int, [_P] + _SETREGION_TAIL),
    "tdx_setregion_strip": (C.c_int, [_P, _P] + _SETREGION_TAIL),
    "tdx_tool_twi": (C.c_int, [C.c_char_p] * 3),
    "tdx_tool_slopearea": (C.c_int, [C.c_char_p] * 3 + [_P]),
    "tdx_tool_slopearearatio": (C.c_int, [C.c_char_p] * 3),
    "tdx_tool_lengtharea": (C.c_int, [C.c_char_p] * 3 + [_P]),
    "tdx_tool_setregion": (C.c_int, [C.c_char_p] * 3 + [_I32]),
}
INDICES_SYMBOLS = tuple(_INDICES_SIGNATURES)
TERRAIN_OUTPUTS = ("twi", "sa", "sar")   # the outputs of tdx_terrain_indices, in the header's order

# name -> (restype, argtypes): the symbols include/taudem_amd_editraster.h declares, the eighth extension header
# EditRaster: ctx, in, nx, ny, [row0,] in_nodata, cols, rows, vals, n, out, stats
_EDITRASTER_SIGNATURES = {
    "tdx_editraster": (C.c_int, [_P, _P, _I64, _I64, _I16, _P, _P, _P, _I64, _P, _P]),
    "tdx_editraster_dev": (C.c_int, [_P, _P, _I64, _I64, _I16, _P, _P, _P, _I64, _P, _P]),
    "tdx_editraster_strip": (C.c_int, [_P, _P, _P, _I64, _I64, _I64, _I16, _P, _P, _P, _I64, _P, _P]),
    "tdx_editraster_read_changes": (C.c_int, [C.c_char_p, _I64, _P, _P, _P, _P]),
    "tdx_tool_editraster": (C.c_int, [C.c_char_p] * 3),
}
EDITRASTER_SYMBOLS = tuple(_EDITRASTER_SIGNATURES)

# name -> (restype, argtypes): the symbols include/taudem_amd_catchoutlets.h declares, the ninth extension header (host code only)
_CATCHOUTLETS_SIGNATURES = {
    "tdx_lines_write": (C.c_int, [C.c_char_p, _P, _P, _P, _I64, _I32, _P, _P, _P, _P, _P]),
    "tdx_lines_read": (C.c_int, [C.c_char_p, _P]),
    "tdx_line_layer_count": (_I64, [_P, _P, _P]),
    "tdx_line_layer_vertices": (None, [_P, _P, _P, _P]),
    "tdx_line_layer_field": (C.c_char_p, [_P, _I32, _P, _P, _P]),
    "tdx_line_layer_value": (C.c_char_p, [_P, _I64, _I32]),
    "tdx_line_layer_free": (None, [_P]),
    # pfile, 4 int32 columns, 7 float64 columns, n_links, mindist, gwstartno, minarea, capacity, out_row, out_x, out_y, out_doutend, out_id, n_out
    "tdx_catchoutlets": (C.c_int, [C.c_char_p] + [_P] * 11 + [_I64, C.c_double, _I32, C.c_double, _I64] + [_P] * 6),
    "tdx_tool_catchoutlets": (C.c_int, [C.c_char_p] * 5 + [C.c_double, C.c_int, C.c_double]),
}
CATCHOUTLETS_SYMBOLS = tuple(_CATCHOUTLETS_SIGNATURES)
# the fields of the stream network layer in the reference's order: name, type (0 Integer, 1 Real), width, decimals (src/streamnet.cpp:163-239); the Real
# ones are, in this order, the nine columns of tdx_streamnet_net_rows
NET_FIELDS = (("LINKNO", 0, 6, 0), ("DSLINKNO", 0, 6, 0), ("USLINKNO1", 0, 6, 0), ("USLINKNO2", 0, 6, 0), ("DSNODEID", 0, 12, 0), ("strmOrder", 0, 6, 0),
              ("Length", 1, 16, 1), ("Magnitude", 0, 6, 0), ("DSContArea", 1, 16, 1), ("strmDrop", 1, 16, 2), ("Slope", 1, 16, 12), ("StraightL", 1, 16, 1),
              ("USContArea", 1, 16, 1), ("WSNO", 0, 6, 0), ("DOUTEND", 1, 16, 1), ("DOUTSTART", 1, 16, 1), ("DOUTMID", 1, 16, 1))
NET_TREE_COLUMN = {"LINKNO": 0, "DSLINKNO": 3, "USLINKNO1": 4, "USLINKNO2": 5, "DSNODEID": 7, "strmOrder": 6, "Magnitude": 8, "WSNO": 0}   # of the -tree file
CATCHOUTLETS_FIELDS = (("LINKNO", 0, 6, 0), ("DSLINKNO", 0, 6, 0), ("USLINKNO1", 0, 6, 0), ("USLINKNO2", 0, 6, 0), ("DOUTEND", 1, 16, 1), ("Id", 0, 10, 0))

# name -> (restype, argtypes): the symbols include/taudem_amd_polygonize.h declares, the tenth extension header
_POLYGONIZE_SIGNATURES = {
    # ctx, w, nx, ny, w_nodata, &polygons, stats
    "tdx_polygonize": (C.c_int, [_P, _P, _I64, _I64, _I32, C.POINTER(_P), _P]),
    "tdx_polygonize_dev": (C.c_int, [_P, _P, _I64, _I64, _I32, C.POINTER(_P), _P]),
    # the same with the rings closed on the device
    "tdx_polygonize_gpu_rings": (C.c_int, [_P, _P, _I64, _I64, _I32, C.POINTER(_P), _P]),
    "tdx_polygonize_gpu_rings_dev": (C.c_int, [_P, _P, _I64, _I64, _I32, C.POINTER(_P), _P]),
    # ctx, comm, w, nx, ny_local, row0, ny_total, w_nodata, &part, stats
    "tdx_polygonize_edges_strip": (C.c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _I32, C.POINTER(_P), _P]),
    # keys, next_keys, ids, n, &part
    "tdx_polygonize_edges_create": (C.c_int, [_P, _P, _P, _I64, C.POINTER(_P)]),
    "tdx_polygonize_edges_count": (_I64, [_P]),
    # part, keys, next_keys, ids, phase_ms
    "tdx_polygonize_edges_copy": (None, [_P] * 5),
    "tdx_polygonize_edges_free": (None, [_P]),
    # parts, n_parts, nx, ny, &polygons
    "tdx_polygonize_rings": (C.c_int, [_P, _I64, _I64, _I64, C.POINTER(_P)]),
    # ctx, parts, n_parts, nx, ny, &polygons, stats
    "tdx_polygonize_rings_gpu": (C.c_int, [_P, _P, _I64, _I64, _I64, C.POINTER(_P), _P]),
    # polygons, ms, &rounds, &workspace_bytes
    "tdx_polygons_ring_phases": (C.c_int, [_P, _P, C.POINTER(_I64), C.POINTER(_I64)]),
    # polygons, &n_polygons, &n_rings, &n_vertices, &n_edges
    "tdx_polygons_count": (_I64, [_P] + [C.POINTER(_I64)] * 4),
    # polygons, ids, cells, poly_first, ring_first, vert_first, vertices, phase_ms
    "tdx_polygons_copy": (None, [_P] * 8),
    "tdx_polygons_free": (None, [_P]),
    # path, polygons, gt
    "tdx_polygons_write": (C.c_int, [C.c_char_p, _P, _P]),
    "tdx_tool_watershedgridtoshp": (C.c_int, [C.c_char_p] * 2),
    "tdx_tool_set_polygon_rings": (C.c_int, [C.c_int]),
}
POLYGONIZE_SYMBOLS = tuple(_POLYGONIZE_SIGNATURES)
POLYGONIZE_PHASES = ("count", "scan", "emit", "download", "rings")
POLYGONIZE_RING_PHASES = ("successor", "validate", "label", "per_ring", "rank", "holes", "order", "scatter")   # of the device ring builder
POLYGONIZE_RINGS = ("host", "device")   # where the rings are closed: the value of tdx_tool_set_polygon_rings is the index

# name -> (restype, argtypes): the symbols include/taudem_amd_regions.h declares, the eleventh extension header
_RG_POLYGONS = [_P, _P, _P, _I64, _P, _P, _I64, _P, _I64]   # x, y, ring_first, n_rings, feature_first, values, n_features, gt, workspace_words
_RG_SOURCE = [_P, _I64, _I64, _P, _I32, _P]                  # src, snx, sny, sgt, src_nodata, gt
_REGIONS_SIGNATURES = {
    # ctx, [comm,] polygons..., nx, ny [ny_local, row0, ny_total], out, ids, &n_ids, phase_ms, &workspace_bytes, stats
    "tdx_regiongrid": (C.c_int, [_P] + _RG_POLYGONS + [_I64, _I64, _P, _P, C.POINTER(_I32), _P, C.POINTER(_I64), _P]),
    "tdx_regiongrid_dev": (C.c_int, [_P] + _RG_POLYGONS + [_I64, _I64, _P, _P, C.POINTER(_I32), _P, C.POINTER(_I64), _P]),
    "tdx_regiongrid_strip": (C.c_int, [_P, _P] + _RG_POLYGONS + [_I64, _I64, _I64, _I64, _P, _P, C.POINTER(_I32), _P, C.POINTER(_I64), _P]),
    # ctx, [comm,] source..., nx, ny [ny_local, row0, ny_total], out, ids, &n_ids, phase_ms, stats
    "tdx_regiongrid_resample": (C.c_int, [_P] + _RG_SOURCE + [_I64, _I64, _P, _P, C.POINTER(_I32), _P, _P]),
    "tdx_regiongrid_resample_dev": (C.c_int, [_P] + _RG_SOURCE + [_I64, _I64, _P, _P, C.POINTER(_I32), _P, _P]),
    "tdx_regiongrid_resample_strip": (C.c_int, [_P, _P] + _RG_SOURCE + [_I64, _I64, _I64, _I64, _P, _P, C.POINTER(_I32), _P, _P]),
    # ctx, [comm,] nx, ny [ny_local, row0, ny_total], out, ids, &n_ids, stats
    "tdx_regiongrid_constant": (C.c_int, [_P, _I64, _I64, _P, _P, C.POINTER(_I32), _P]),
    "tdx_regiongrid_constant_dev": (C.c_int, [_P, _I64, _I64, _P, _P, C.POINTER(_I32), _P]),
    "tdx_regiongrid_constant_strip": (C.c_int, [_P, _P, _I64, _I64, _I64, _I64, _P, _P, C.POINTER(_I32), _P]),
    # path, ids, n_ids, seven_texts
    "tdx_regiongrid_write_calpar": (C.c_int, [C.c_char_p, _P, _I32, _P]),
    # path, &layer
    "tdx_polygon_layer_read": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    # layer, &n_rings, &n_vertices, &n_fields
    "tdx_polygon_layer_count": (_I64, [_P] + [C.POINTER(_I64)] * 3),
    # layer, feature_first, ring_first, x, y
    "tdx_polygon_layer_copy": (None, [_P] * 5),
    "tdx_polygon_layer_field": (C.c_char_p, [_P, _I64]),
    "tdx_polygon_layer_value": (C.c_char_p, [_P, _I64, _I64]),
    # layer, field, values
    "tdx_polygon_layer_values": (C.c_int, [_P, C.c_char_p, _P]),
    "tdx_polygon_layer_free": (None, [_P]),
    # dem, parreg, att, parreg_in, shp, shp_att_name, seven_texts
    "tdx_tool_siregiontool": (C.c_int, [C.c_char_p] * 6 + [_P]),
}
REGIONS_SYMBOLS = tuple(_REGIONS_SIGNATURES)
REGIONGRID_PHASES = ("prepare", "cross", "fill", "write")
REGIONGRID_MAX_IDS = 32767

_lib = None


def load():
    """Load the shared library (once).  Raises ImportError with a build hint if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C taudem_amd/csrc` (hipcc, --offload-arch=gfx950). taudem_amd has no CPU fallback."
        )
    # One HIP/HSA runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64.
    # If torch is importable, load it FIRST so that this library binds to the already-loaded runtime
    # (same SONAME) instead of pulling /opt/rocm's copy in beside it - with two HSA runtimes in one
    # process whichever initialises second sees "no HIP GPUs".  torch is plumbing here (device memory,
    # streams, torch.distributed), not a dependency of the C ABI itself.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch-less hosts use the system ROCm runtime
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**_SIGNATURES, **_DROPAN_SIGNATURES, **_PEUKER_SIGNATURES, **_AD8_SIGNATURES, **_STREAMNET_SIGNATURES,
                                   **_OUTLETS_SIGNATURES, **_SINMAP_SIGNATURES, **_INDICES_SIGNATURES, **_EDITRASTER_SIGNATURES, **_CATCHOUTLETS_SIGNATURES,
                                   **_POLYGONIZE_SIGNATURES, **_REGIONS_SIGNATURES}.items():
        fn = getattr(lib, name)   # AttributeError = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class TdxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"taudem_amd error {code}: {msg}")
        self.code = code


def last_error(ctx=None):
    s = load().tdx_last_error(ctx)
    return s.decode("utf-8", "replace") if s else ""


def check(rc, ctx=None):
    if rc != TDX_OK:
        raise TdxError(rc, last_error(ctx) or last_error(None))
