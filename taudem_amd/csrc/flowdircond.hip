// FlowDirCond (flowdircond, src/flowdircond.cpp:54-252) on gfx950: the elevation raster conditioned along the D8 directions - every cell
// becomes the minimum of its own value and the conditioned values of the cells that drain into it.
//
// The reference is the Kahn queue of initNeighborD8up (src/commonLib.cpp:251-282) from the ridges downstream: the forward D8 tile sweep
// of d8_sweep.hpp with the set-up of the AreaD8 family (codes 0..8 take part; a p == 0 neighbour is counted at k == 4 and never drains:
// INFO_DEAD) and one more value policy.
//   FlowDirCondAlg: a float record.  A cell whose z is not nodata folds, in k = 1..8 order, `if (z(n) < zval) zval = z(n)` over the
//     neighbours that have a code 1..8, drain into it and whose (already conditioned) z is not nodata (src/flowdircond.cpp:151-172); a
//     cell with nodata z keeps it, and releases its receiver all the same.
// Cells that are never evaluated - no valid code, dead, on or below a cycle - keep their INPUT value: the work array starts as the
// pending pattern on participating cells and z elsewhere, and what is still pending at the end gets z back.
#include "context.hpp"
#include "d8_sweep.hpp"
#include "device_common.hpp"

namespace {
using namespace tdxk;

struct FlowDirCondAlg {   // src/flowdircond.cpp:151-172
    using Cell = float;
    using Aux = float;                              // the cell's own input z
    static constexpr bool HAS_AUX = true, HAS_DIST = false, HAS_ROWS = false;
    static constexpr int kBulkSweeps = d8sweep::BULK_SWEEPS_D8;
    static constexpr unsigned kBulkUntil = 16;
    static constexpr int kMinWaves32 = 4;
    static constexpr int kMaxRelease = 1;
    static __device__ __forceinline__ unsigned rel_mask(unsigned inf) { const unsigned code = (inf >> 9) & 15u; return (code >= 1u && code <= 8u) ? 1u << (code - 1u) : 0u; }
    float z_nodata;
    static __device__ __forceinline__ float head(float c) { return c; }
    static __host__ __device__ __forceinline__ float outside() { return TDX_ANG_NODATA; }   // (never read: cells outside the raster are nobody's contributor)
    template <class L>
    __device__ __forceinline__ void eval(L& S, int c, int cl, int, unsigned inf, const Cell (&nb)[9]) const {
        float a = S.aux[c];
        if (!is_nodata_f(a, z_nodata)) {
#pragma unroll
            for (int k = 1; k <= 8; k++) {
                if (!((inf >> (16 + k - 1)) & 1u)) continue;   // code 1..8 and drains into the cell (a p == 0 neighbour makes the cell dead: never evaluated)
                const float v = nb[k];
                if (!is_nodata_f(v, z_nodata) && v < a) a = v;
            }
        }
        S.v[cl] = a;
    }
};

__global__ __launch_bounds__(256) void fdc_init_kernel(const uint32_t* __restrict__ info, const float* __restrict__ z, float* __restrict__ v, size_t first, size_t n) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < first + n) v[i] = (info[i] & d8sweep::INFO_PART) ? __uint_as_float(d8sweep::PENDING_BITS) : z[i];
}
__global__ __launch_bounds__(256) void fdc_finish_kernel(const float* __restrict__ z, float* __restrict__ v, size_t first, size_t n) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < first + n && d8sweep::pending(v[i])) v[i] = z[i];
}

int fdc_impl(tdx_context* ctx, const Strip& st, int16_t* d_p, int16_t p_nodata, const float* d_z, float z_nodata, float* d_out, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int inx = st.nx, iny = st.ny_arr;
    const size_t n = size_t(inx) * size_t(iny);
    const size_t first = size_t(st.y0) * size_t(inx), nown = size_t(st.y1 - st.y0) * size_t(inx);
    uint32_t* info = static_cast<uint32_t*>(ctx->scratch(TDX_S_A, n * 4));
    unsigned long long* counts = static_cast<unsigned long long*>(ctx->scratch(TDX_S_M, size_t(tilek::COUNT_RING) * 16));
    if (!info || !counts) return TDX_ERR_NOMEM;
    ctx->begin_call(stats);
    strip_mark(ctx, st, "flowdircond");
    int rc = strip_exchange<int16_t>(ctx, st, d_p, p_nodata);   // flowData->share()
    if (rc != TDX_OK) return rc;
    {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        hipLaunchKernelGGL(d8sweep::setup_kernel, dim3((inx + 63) / 64, (iny + 3) / 4), dim3(256), 0, s, d_p, inx, iny, p_nodata, 0, nullptr, 0, nullptr, info);
        hipLaunchKernelGGL(fdc_init_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, info, d_z, d_out, first, nown);
        if (stats) stats->launches[TDX_K_STENCIL] += 2;
    }
    rc = strip_exchange<float>(ctx, st, d_out, FlowDirCondAlg::outside());
    if (rc != TDX_OK) return rc;
    int64_t rounds = 0, launches = 0, outer = 1;
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        d8sweep::Arrays<FlowDirCondAlg> A{d_out, d_z, nullptr, nullptr, info};
        rc = d8sweep::run(ctx, st, FlowDirCondAlg{z_nodata}, A, counts, &rounds, &launches, &outer);
        if (rc != TDX_OK) return rc;
        hipLaunchKernelGGL(fdc_finish_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, d_z, d_out, first, nown);   // never evaluated: the input value
        if (stats) stats->launches[TDX_K_ACCUM] += launches;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    return TDX_OK;
}

}  // namespace

// the argument test of the _dev (halo 0) and _strip (halo 2: the strip's two halo rows) entry points
static int fdc_check(tdx_context* ctx, const void* p, const void* z, const void* zfdc, int64_t nx, int64_t ny, int64_t halo, const char* who) {
    if (!ctx || !p || !z || !zfdc || z == zfdc || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}

extern "C" int tdx_flowdircond_dev(tdx_context* ctx, const int16_t* d_p, int64_t nx, int64_t ny, int16_t p_nodata, const float* d_z, float z_nodata, float* d_zfdc,
                                   tdx_stats* stats) {
    if (int rc = fdc_check(ctx, d_p, d_z, d_zfdc, nx, ny, 0, "tdx_flowdircond_dev: bad argument")) return rc;
    return fdc_impl(ctx, strip_single(int(nx), int(ny)), const_cast<int16_t*>(d_p), p_nodata, d_z, z_nodata, d_zfdc, stats);
}
extern "C" int tdx_flowdircond_strip(tdx_context* ctx, const tdx_comm* comm, int16_t* d_p, int64_t nx, int64_t ny_local, int16_t p_nodata, const float* d_z,
                                     float z_nodata, float* d_zfdc, tdx_stats* stats) {
    if (int rc = fdc_check(ctx, d_p, d_z, d_zfdc, nx, ny_local, 2, "tdx_flowdircond_strip: bad argument")) return rc;
    return fdc_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_p, p_nodata, d_z, z_nodata, d_zfdc, stats);
}
extern "C" int tdx_flowdircond(tdx_context* ctx, const int16_t* p, int64_t nx, int64_t ny, int16_t p_nodata, const float* z, float z_nodata, float* zfdc,
                               tdx_stats* stats) {
    if (!ctx || !p || !z || !zfdc || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_flowdircond: bad argument");
    HostCall h(ctx, nx, ny);
    int16_t* d_p = h.in(TDX_S_IO0, p);
    float* d_o = h.out(TDX_S_IO1, zfdc);
    float* d_z = h.in(TDX_S_IO2, z);
    if (h.error) return h.error;
    return h.finish(tdx_flowdircond_dev(ctx, d_p, nx, ny, p_nodata, d_z, z_nodata, d_o, stats));
}
