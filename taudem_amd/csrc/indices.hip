// The terrain-index tools: TWI (src/TWI.cpp:108-123), SlopeArea (src/SlopeArea.cpp:112-123), SlopeAreaRatio (src/SlopeAreaRatio.cpp:108-119), LengthArea
// (src/LengthArea.cpp:110-120) and SetRegion (src/SetRegion.cpp:140-166).  The first four are functions of a cell's own inputs, so the raster is one flat array
// of cells as in sinmap.hip: a lane takes four consecutive cells with 16-byte accesses (8-byte for int16), an array whose first cell is not aligned for that
// and the last, partial group of four take element accesses in the same kernel.  SetRegion streams the same way and looks at the eight neighbours of p only
// on the lanes whose cell is nodata in p and in gw.
//
//   terrain_index_kernel<MASK>   slp, sca -> any non-empty subset of twi (1), sa (2), sar (4): one instantiation per subset, a one-output call moves 12 B/cell,
//                                the three-output call 20 B/cell
//   lengtharea_kernel            plen, ad8 -> ss (int16)
//   setregion_kernel             p (int16), gw (int32) -> out (int32)
//
// The arithmetic contract (include/taudem_amd_indices.h, DESIGN.md "Terrain indices"): what the reference computes with logf / powf is the correctly rounded
// float here, from an evaluation in double rounded once (ti_log, ti_pow); everything around the library call is the reference's float arithmetic in its order (the library is
// built with -ffp-contract=off).
#include <algorithm>
#include <cstdlib>

#include "context.hpp"
#include "device_common.hpp"
#include "strips.hpp"

namespace {

enum { TI_TWI = 1, TI_SA = 2, TI_SAR = 4 };

struct TiParams {
    float slp_nodata, sca_nodata;
    float m, n;   // SlopeArea's exponents
};

__device__ __forceinline__ float ti_log(float q) { return float(log(double(q))); }
// RN_float(x^e).  e == 0, 1, 2 - the reference's defaults among them - need no library call: x * x is exact in double, so the one rounding to float is the
// correct one, ties included.  Which branch is taken is uniform in the launch.  Every other e takes pow in double: exp2(e * log2 x) in double keeps the
// contract as well (error under 2^-45) but took 1.55 x the time of pow in lengtharea_kernel at 16384^2 (docs/experiments_indices.md).
__device__ __forceinline__ float ti_pow(float x, float e) {
    if (e == 1.0f) return x;
    if (e == 0.0f) return 1.0f;
    if (e == 2.0f) return float(double(x) * double(x));
    return float(pow(double(x), double(e)));
}

// the reference's LONG_TYPE read of a float file (GDALCopyWords as oracle/gdal_shim reads it: NaN -> 0, halves away from zero, clamped)
__device__ __forceinline__ int32_t ti_long_of(float a) {
    double v = double(a);
    if (v != v) return 0;
    v = (v >= 0) ? floor(v + 0.5) : ceil(v - 0.5);
    if (v > 2147483647.0) return 2147483647;
    if (v < -2147483648.0) return int32_t(-2147483647 - 1);
    return int32_t(v);
}

template <class T, class V4>
__device__ __forceinline__ void ti_load4(const T* __restrict__ p, unsigned long long c, int m, bool vec, T (&v)[4]) {
    if (vec && m == 4) {
        const V4 q = *reinterpret_cast<const V4*>(p + c);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = k < m ? p[c + k] : T(0);
    }
}

template <class T, class V4>
__device__ __forceinline__ void ti_store4(T* __restrict__ p, unsigned long long c, int m, bool vec, const T (&v)[4]) {
    if (vec && m == 4) {
        V4 q;
        q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        *reinterpret_cast<V4*>(p + c) = q;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) if (k < m) p[c + k] = v[k];
    }
}

// alignment bits of a launch: set = the array's first cell is aligned for the vector access
enum { TI_AL_IN0 = 1, TI_AL_IN1 = 2, TI_AL_OUT0 = 4, TI_AL_OUT1 = 8, TI_AL_OUT2 = 16 };

template <int MASK>
__global__ __launch_bounds__(256) void terrain_index_kernel(const float* __restrict__ slp, const float* __restrict__ sca, unsigned long long n, unsigned al, TiParams P,
                                                            float* __restrict__ twi, float* __restrict__ sa, float* __restrict__ sar) {
    const unsigned long long c = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) * 4ull;
    if (c >= n) return;
    const int m = n - c < 4ull ? int(n - c) : 4;
    float s[4], a[4], vt[4], vp[4], vr[4];
    ti_load4<float, float4>(slp, c, m, al & TI_AL_IN0, s);
    ti_load4<float, float4>(sca, c, m, al & TI_AL_IN1, a);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool sca_nd = tdxk::is_nodata_f(a[k], P.sca_nodata);
        if (MASK & TI_TWI) {
            vt[k] = -1.0f;
            if (!sca_nd && !tdxk::is_nodata_f(s[k], P.slp_nodata) && s[k] > 0.0f && a[k] > 0.0f) vt[k] = ti_log(a[k] / s[k]);
        }
        if (MASK & TI_SA) {
            vp[k] = -1.0f;
            if (s[k] >= 0.0f && a[k] >= 0.0f) vp[k] = ti_pow(s[k], P.m) * ti_pow(a[k], P.n);
        }
        if (MASK & TI_SAR) vr[k] = sca_nd ? -1.0f : s[k] / a[k];
    }
    if (MASK & TI_TWI) ti_store4<float, float4>(twi, c, m, al & TI_AL_OUT0, vt);
    if (MASK & TI_SA) ti_store4<float, float4>(sa, c, m, al & TI_AL_OUT1, vp);
    if (MASK & TI_SAR) ti_store4<float, float4>(sar, c, m, al & TI_AL_OUT2, vr);
}

__global__ __launch_bounds__(256) void lengtharea_kernel(const float* __restrict__ plen, const float* __restrict__ ad8, unsigned long long n, unsigned al, float M, float y,
                                                         int16_t* __restrict__ ss) {
    const unsigned long long c = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) * 4ull;
    if (c >= n) return;
    const int m = n - c < 4ull ? int(n - c) : 4;
    float l[4], a[4];
    int16_t v[4];
    ti_load4<float, float4>(plen, c, m, al & TI_AL_IN0, l);
    ti_load4<float, float4>(ad8, c, m, al & TI_AL_IN1, a);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = int16_t(-32768);   // not written by the reference: the partition's initial value
        if (l[k] >= 0.0f) v[k] = (float(ti_long_of(a[k])) >= M * ti_pow(l[k], y)) ? int16_t(1) : int16_t(0);
    }
    ti_store4<int16_t, short4>(ss, c, m, al & TI_AL_OUT0, v);
}

// p: the whole array of `rows` rows (a strip: with its halo rows), read from row y0 on; gw, out: at the first owned row y0; n owned cells
__global__ __launch_bounds__(256) void setregion_kernel(const int16_t* __restrict__ p, const int32_t* __restrict__ gw, int nx, int rows, int y0, unsigned long long n,
                                                        unsigned al, int16_t p_nodata, int32_t gw_nodata, int32_t region_id, int32_t* __restrict__ out) {
    const unsigned long long c = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) * 4ull;
    if (c >= n) return;
    const int m = n - c < 4ull ? int(n - c) : 4;
    const unsigned long long off = (unsigned long long)y0 * (unsigned long long)nx;
    int16_t d[4];
    int32_t g[4], v[4];
    ti_load4<int16_t, short4>(p + off, c, m, al & TI_AL_IN0, d);
    ti_load4<int32_t, int4>(gw, c, m, al & TI_AL_IN1, g);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = region_id;
        if (k < m && g[k] == gw_nodata && tdxk::is_nodata_s(d[k], p_nodata)) {
            v[k] = -2147483647;   // MISSINGLONG
            const unsigned cell = unsigned(c) + unsigned(k);   // < n <= 2^32 - 1
            const int j = y0 + int(cell / unsigned(nx)), i = int(cell % unsigned(nx));
            for (int q = 1; q <= 8; q++) {
                const int in = i + tdxk::d1(q), jn = j + tdxk::d2(q);
                if (in < 0 || in >= nx || jn < 0 || jn >= rows) continue;
                const int16_t dn = p[size_t(jn) * size_t(nx) + size_t(in)];
                if (!tdxk::is_nodata_s(dn, p_nodata) && dn > 0 && abs(int(dn) - q) == 4) { v[k] = region_id; break; }
            }
        }
    }
    ti_store4<int32_t, int4>(out, c, m, al & TI_AL_OUT0, v);
}

bool ti_aligned(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }
unsigned ti_grid(unsigned long long n) { return unsigned((n + 1023ull) / 1024ull); }   // n < 2^32: at most 2^22 blocks

template <int MASK>
void ti_launch(hipStream_t s, const float* slp, const float* sca, unsigned long long n, unsigned al, const TiParams& P, float* twi, float* sa, float* sar) {
    hipLaunchKernelGGL(terrain_index_kernel<MASK>, dim3(ti_grid(n)), dim3(256), 0, s, slp, sca, n, al, P, twi, sa, sar);
}

// One strip (or the whole raster, a strip without halo rows): the cells of the owned rows
int terrain_impl(tdx_context* ctx, const Strip& st, const float* d_slp, const float* d_sca, const TiParams& P, float* d_twi, float* d_sa, float* d_sar, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t off = size_t(st.y0) * size_t(st.nx);
    const unsigned long long n = (unsigned long long)(st.y1 - st.y0) * (unsigned long long)st.nx;
    ctx->begin_call(stats);
    strip_mark(ctx, st, "terrain_indices");
    ctx->phase = "cells";
    const float *slp = d_slp + off, *sca = d_sca + off;
    float *twi = d_twi ? d_twi + off : nullptr, *sa = d_sa ? d_sa + off : nullptr, *sar = d_sar ? d_sar + off : nullptr;
    const unsigned al = (ti_aligned(slp, 16) ? TI_AL_IN0 : 0) | (ti_aligned(sca, 16) ? TI_AL_IN1 : 0) | (ti_aligned(twi, 16) ? TI_AL_OUT0 : 0) |
                        (ti_aligned(sa, 16) ? TI_AL_OUT1 : 0) | (ti_aligned(sar, 16) ? TI_AL_OUT2 : 0);
    {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        switch ((twi ? TI_TWI : 0) | (sa ? TI_SA : 0) | (sar ? TI_SAR : 0)) {
        case 1: ti_launch<1>(s, slp, sca, n, al, P, twi, sa, sar); break;
        case 2: ti_launch<2>(s, slp, sca, n, al, P, twi, sa, sar); break;
        case 3: ti_launch<3>(s, slp, sca, n, al, P, twi, sa, sar); break;
        case 4: ti_launch<4>(s, slp, sca, n, al, P, twi, sa, sar); break;
        case 5: ti_launch<5>(s, slp, sca, n, al, P, twi, sa, sar); break;
        case 6: ti_launch<6>(s, slp, sca, n, al, P, twi, sa, sar); break;
        default: ti_launch<7>(s, slp, sca, n, al, P, twi, sa, sar); break;
        }
        if (stats) stats->launches[TDX_K_STENCIL]++;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    ctx->end_call();
    return TDX_OK;
}

int lengtharea_impl(tdx_context* ctx, const Strip& st, const float* d_plen, const float* d_ad8, float M, float y, int16_t* d_ss, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t off = size_t(st.y0) * size_t(st.nx);
    const unsigned long long n = (unsigned long long)(st.y1 - st.y0) * (unsigned long long)st.nx;
    ctx->begin_call(stats);
    strip_mark(ctx, st, "lengtharea");
    ctx->phase = "cells";
    const float *plen = d_plen + off, *ad8 = d_ad8 + off;
    int16_t* ss = d_ss + off;
    const unsigned al = (ti_aligned(plen, 16) ? TI_AL_IN0 : 0) | (ti_aligned(ad8, 16) ? TI_AL_IN1 : 0) | (ti_aligned(ss, 8) ? TI_AL_OUT0 : 0);
    {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        hipLaunchKernelGGL(lengtharea_kernel, dim3(ti_grid(n)), dim3(256), 0, s, plen, ad8, n, al, M, y, ss);
        if (stats) stats->launches[TDX_K_STENCIL]++;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    ctx->end_call();
    return TDX_OK;
}

int setregion_impl(tdx_context* ctx, const Strip& st, int16_t* d_p, const int32_t* d_gw, int16_t p_nodata, int32_t gw_nodata, int32_t region_id, int32_t* d_out,
                   tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t off = size_t(st.y0) * size_t(st.nx);
    const unsigned long long n = (unsigned long long)(st.y1 - st.y0) * (unsigned long long)st.nx;
    ctx->begin_call(stats);
    strip_mark(ctx, st, "setregion");
    ctx->phase = "cells";
    if (int rc = strip_exchange<int16_t>(ctx, st, d_p, p_nodata)) return rc;   // the reference's pData->share(); beyond the raster: nodata, which no test takes
    const int32_t* gw = d_gw + off;
    int32_t* out = d_out + off;
    const unsigned al = (ti_aligned(d_p + off, 8) ? TI_AL_IN0 : 0) | (ti_aligned(gw, 16) ? TI_AL_IN1 : 0) | (ti_aligned(out, 16) ? TI_AL_OUT0 : 0);
    {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        hipLaunchKernelGGL(setregion_kernel, dim3(ti_grid(n)), dim3(256), 0, s, d_p, gw, st.nx, st.ny_arr, st.y0, n, al, p_nodata, gw_nodata, region_id, out);
        if (stats) stats->launches[TDX_K_STENCIL]++;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    ctx->end_call();
    return TDX_OK;
}

int ti_check(tdx_context* ctx, bool have, int64_t nx, int64_t ny, int64_t halo, const char* who) {
    if (!ctx || !have || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}

}  // namespace

extern "C" int tdx_terrain_indices_dev(tdx_context* ctx, const float* d_slp, const float* d_sca, int64_t nx, int64_t ny, float slp_nodata, float sca_nodata, float m,
                                       float n, float* d_twi, float* d_sa, float* d_sar, tdx_stats* stats) {
    if (int rc = ti_check(ctx, d_slp && d_sca && (d_twi || d_sa || d_sar), nx, ny, 0, "tdx_terrain_indices_dev: bad argument")) return rc;
    return terrain_impl(ctx, strip_single(int(nx), int(ny)), d_slp, d_sca, TiParams{slp_nodata, sca_nodata, m, n}, d_twi, d_sa, d_sar, stats);
}

extern "C" int tdx_terrain_indices_strip(tdx_context* ctx, const tdx_comm* comm, const float* d_slp, const float* d_sca, int64_t nx, int64_t ny_local, float slp_nodata,
                                         float sca_nodata, float m, float n, float* d_twi, float* d_sa, float* d_sar, tdx_stats* stats) {
    if (int rc = ti_check(ctx, d_slp && d_sca && (d_twi || d_sa || d_sar), nx, ny_local, 2, "tdx_terrain_indices_strip: bad argument")) return rc;
    return terrain_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_slp, d_sca, TiParams{slp_nodata, sca_nodata, m, n}, d_twi, d_sa, d_sar, stats);
}

extern "C" int tdx_terrain_indices(tdx_context* ctx, const float* slp, const float* sca, int64_t nx, int64_t ny, float slp_nodata, float sca_nodata, float m, float n,
                                   float* twi, float* sa, float* sar, tdx_stats* stats) {
    if (!ctx || !slp || !sca || !(twi || sa || sar) || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_terrain_indices: bad argument");
    HostCall h(ctx, nx, ny);
    const float* d_slp = h.in(TDX_S_IO0, slp);
    const float* d_sca = h.in(TDX_S_IO1, sca);
    float* d_twi = h.out(TDX_S_E, twi);   // each optional
    float* d_sa = h.out(TDX_S_F, sa);
    float* d_sar = h.out(TDX_S_IO2, sar);
    if (h.error) return h.error;
    return h.finish(tdx_terrain_indices_dev(ctx, d_slp, d_sca, nx, ny, slp_nodata, sca_nodata, m, n, d_twi, d_sa, d_sar, stats));
}

extern "C" int tdx_lengtharea_dev(tdx_context* ctx, const float* d_plen, const float* d_ad8, int64_t nx, int64_t ny, float M, float y, int16_t* d_ss, tdx_stats* stats) {
    if (int rc = ti_check(ctx, d_plen && d_ad8 && d_ss, nx, ny, 0, "tdx_lengtharea_dev: bad argument")) return rc;
    return lengtharea_impl(ctx, strip_single(int(nx), int(ny)), d_plen, d_ad8, M, y, d_ss, stats);
}

extern "C" int tdx_lengtharea_strip(tdx_context* ctx, const tdx_comm* comm, const float* d_plen, const float* d_ad8, int64_t nx, int64_t ny_local, float M, float y,
                                    int16_t* d_ss, tdx_stats* stats) {
    if (int rc = ti_check(ctx, d_plen && d_ad8 && d_ss, nx, ny_local, 2, "tdx_lengtharea_strip: bad argument")) return rc;
    return lengtharea_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_plen, d_ad8, M, y, d_ss, stats);
}

extern "C" int tdx_lengtharea(tdx_context* ctx, const float* plen, const float* ad8, int64_t nx, int64_t ny, float M, float y, int16_t* ss, tdx_stats* stats) {
    if (!ctx || !plen || !ad8 || !ss || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_lengtharea: bad argument");
    HostCall h(ctx, nx, ny);
    const float* d_plen = h.in(TDX_S_IO0, plen);
    const float* d_ad8 = h.in(TDX_S_IO1, ad8);
    int16_t* d_ss = h.out(TDX_S_E, ss);
    if (h.error) return h.error;
    return h.finish(tdx_lengtharea_dev(ctx, d_plen, d_ad8, nx, ny, M, y, d_ss, stats));
}

extern "C" int tdx_setregion_dev(tdx_context* ctx, const int16_t* d_p, const int32_t* d_gw, int64_t nx, int64_t ny, int16_t p_nodata, int32_t gw_nodata, int32_t region_id,
                                 int32_t* d_out, tdx_stats* stats) {
    if (int rc = ti_check(ctx, d_p && d_gw && d_out, nx, ny, 0, "tdx_setregion_dev: bad argument")) return rc;
    // (without halo rows strip_exchange writes nothing: p is only read)
    return setregion_impl(ctx, strip_single(int(nx), int(ny)), const_cast<int16_t*>(d_p), d_gw, p_nodata, gw_nodata, region_id, d_out, stats);
}

extern "C" int tdx_setregion_strip(tdx_context* ctx, const tdx_comm* comm, int16_t* d_p, const int32_t* d_gw, int64_t nx, int64_t ny_local, int16_t p_nodata,
                                   int32_t gw_nodata, int32_t region_id, int32_t* d_out, tdx_stats* stats) {
    if (int rc = ti_check(ctx, d_p && d_gw && d_out, nx, ny_local, 2, "tdx_setregion_strip: bad argument")) return rc;
    return setregion_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_p, d_gw, p_nodata, gw_nodata, region_id, d_out, stats);
}

extern "C" int tdx_setregion(tdx_context* ctx, const int16_t* p, const int32_t* gw, int64_t nx, int64_t ny, int16_t p_nodata, int32_t gw_nodata, int32_t region_id,
                             int32_t* out, tdx_stats* stats) {
    if (!ctx || !p || !gw || !out || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_setregion: bad argument");
    HostCall h(ctx, nx, ny);
    const int16_t* d_p = h.in(TDX_S_IO0, p);
    const int32_t* d_gw = h.in(TDX_S_IO1, gw);
    int32_t* d_out = h.out(TDX_S_E, out);
    if (h.error) return h.error;
    return h.finish(tdx_setregion_dev(ctx, d_p, d_gw, nx, ny, p_nodata, gw_nodata, region_id, d_out, stats));
}
