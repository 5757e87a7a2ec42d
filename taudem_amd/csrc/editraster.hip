// EditRaster (src/EditRaster.cpp:111-144): a copy of an int16 raster in which the input's nodata value becomes -32768, then a handful of cells set to new values.
//
//   editraster_copy_kernel      in -> out, 2 + 2 bytes per cell: a lane takes eight consecutive cells with one 16-byte load and one 16-byte store and recodes
//                               them as packed halves of four words; arrays whose first cell is not 16-byte aligned (a strip of a raster with an odd nx) and
//                               the last, partial group of eight take element accesses in the same kernel
//   editraster_scatter_kernel   one lane per change, after the copy in stream order
//
// The reference applies the changes in file order, so the last change of a cell holds.  That order is settled on the host (editraster_changes.cpp keeps the
// last change per cell): the scatter has one writer per cell and no ordering to keep.  in == out is allowed: a cell is read and written by the same lane, which
// is why neither pointer is __restrict__.
#include <vector>

#include "context.hpp"
#include "device_common.hpp"
#include "editraster_changes.hpp"
#include "strips.hpp"

namespace {

// two cells in one word
__device__ __forceinline__ uint32_t er_recode2(uint32_t w, uint32_t nd) {
    uint32_t lo = w & 0xffffu, hi = w >> 16;
    if (lo == nd) lo = 0x8000u;
    if (hi == nd) hi = 0x8000u;
    return lo | (hi << 16);
}

__global__ __launch_bounds__(256) void editraster_copy_kernel(const int16_t* in, int16_t* out, unsigned long long n, bool vec, int16_t nodata) {
    const unsigned long long c = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) * 8ull;
    if (c >= n) return;
    if (vec && n - c >= 8ull) {
        const uint32_t nd = uint32_t(uint16_t(nodata));
        uint4 q = *reinterpret_cast<const uint4*>(in + c);
        q.x = er_recode2(q.x, nd); q.y = er_recode2(q.y, nd); q.z = er_recode2(q.z, nd); q.w = er_recode2(q.w, nd);
        *reinterpret_cast<uint4*>(out + c) = q;
    } else {
        const int m = n - c < 8ull ? int(n - c) : 8;
        int16_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = k < m ? in[c + k] : int16_t(0);
#pragma unroll
        for (int k = 0; k < 8; k++) if (k < m) out[c + k] = tdxk::is_nodata_s(v[k], nodata) ? int16_t(-32768) : v[k];
    }
}

// cell[i] < the cells of the owned rows, no two equal (select_raster_changes)
__global__ __launch_bounds__(256) void editraster_scatter_kernel(int16_t* __restrict__ out, const uint32_t* __restrict__ cell, const int16_t* __restrict__ val, unsigned m) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < m) out[cell[i]] = val[i];
}

bool er_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; }

// One strip (or the whole raster, a strip without halo rows) whose first owned row is global row row_lo
int editraster_impl(tdx_context* ctx, const Strip& st, int64_t row_lo, const int16_t* d_in, int16_t in_nodata, const int32_t* cols, const int32_t* rows, const int32_t* vals,
                    int64_t n_changes, int16_t* d_out, tdx_stats* stats, const char* range_msg) {
    std::vector<uint32_t> cell;
    std::vector<int16_t> val;
    if (!tdx::select_raster_changes(cols, rows, vals, n_changes, st.nx, row_lo, row_lo + (st.y1 - st.y0), cell, val)) return tdx_fail(ctx, TDX_ERR_ARG, range_msg);
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t off = size_t(st.y0) * size_t(st.nx), m = cell.size();
    const unsigned long long n = (unsigned long long)(st.y1 - st.y0) * (unsigned long long)st.nx;
    ctx->begin_call(stats);
    strip_mark(ctx, st, "editraster");
    ctx->phase = "cells";
    const int16_t* in = d_in + off;
    int16_t* out = d_out + off;
    uint32_t* d_cell = nullptr;
    int16_t* d_val = nullptr;
    if (m) {
        d_cell = static_cast<uint32_t*>(ctx->scratch(TDX_S_K, m * 6 + 16));
        if (!d_cell) return tdx_fail(ctx, TDX_ERR_NOMEM, "editraster: out of device memory");
        d_val = reinterpret_cast<int16_t*>(d_cell + m);
        // (cell and val live until end_call() has waited for the stream)
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_cell, cell.data(), m * 4, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_val, val.data(), m * 2, hipMemcpyHostToDevice, s));
    }
    {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        hipLaunchKernelGGL(editraster_copy_kernel, dim3(unsigned((n + 2047ull) / 2048ull)), dim3(256), 0, s, in, out, n, er_aligned(in) && er_aligned(out), in_nodata);
        if (m) hipLaunchKernelGGL(editraster_scatter_kernel, dim3(tdx_blocks_for(m, 256)), dim3(256), 0, s, out, d_cell, d_val, unsigned(m));
        if (stats) stats->launches[TDX_K_STENCIL] += m ? 2 : 1;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    ctx->end_call();
    return TDX_OK;
}

bool er_bad(const void* in, const void* out, int64_t nx, int64_t ny, const void* cols, const void* rows, const void* vals, int64_t n) {
    return !in || !out || nx <= 0 || ny <= 0 || n < 0 || n > 0x7fffffff || (n > 0 && (!cols || !rows || !vals));
}

}  // namespace

extern "C" int tdx_editraster_dev(tdx_context* ctx, const int16_t* d_in, int64_t nx, int64_t ny, int16_t in_nodata, const int32_t* cols, const int32_t* rows,
                                  const int32_t* vals, int64_t n, int16_t* d_out, tdx_stats* stats) {
    if (!ctx || er_bad(d_in, d_out, nx, ny, cols, rows, vals, n)) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_editraster_dev: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    return editraster_impl(ctx, strip_single(int(nx), int(ny)), 0, d_in, in_nodata, cols, rows, vals, n, d_out, stats, "tdx_editraster_dev: a value outside -32768 .. 32767");
}

extern "C" int tdx_editraster_strip(tdx_context* ctx, const tdx_comm* comm, const int16_t* d_in, int64_t nx, int64_t ny_local, int64_t row0, int16_t in_nodata,
                                    const int32_t* cols, const int32_t* rows, const int32_t* vals, int64_t n, int16_t* d_out, tdx_stats* stats) {
    if (!ctx || er_bad(d_in, d_out, nx, ny_local, cols, rows, vals, n) || row0 < 0 || row0 + ny_local > 0x7ffffff0)
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_editraster_strip: bad argument");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    return editraster_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), row0, d_in, in_nodata, cols, rows, vals, n, d_out, stats,
                           "tdx_editraster_strip: a value outside -32768 .. 32767");
}

extern "C" int tdx_editraster(tdx_context* ctx, const int16_t* in, int64_t nx, int64_t ny, int16_t in_nodata, const int32_t* cols, const int32_t* rows, const int32_t* vals,
                              int64_t n, int16_t* out, tdx_stats* stats) {
    if (!ctx || er_bad(in, out, nx, ny, cols, rows, vals, n)) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_editraster: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    for (int64_t k = 0; k < n; k++)   // before the upload
        if (vals[k] < -32768 || vals[k] > 32767) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_editraster: a value outside -32768 .. 32767");
    HostCall h(ctx, nx, ny);
    const int16_t* d_in = h.in(TDX_S_IO0, in);
    int16_t* d_out = h.out(TDX_S_E, out);
    if (h.error) return h.error;
    return h.finish(tdx_editraster_dev(ctx, d_in, nx, ny, in_nodata, cols, rows, vals, n, d_out, stats));
}
