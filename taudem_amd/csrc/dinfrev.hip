// DinfUpDependence (depgrd, src/DinfUpDependence.cpp:52-272) and DinfRevAccum (dsaccum, src/DinfRevAccum.cpp:51-290) on gfx950 -
// the D-infinity flow-algebra tools that sweep the dependency graph of AreaDinf in REVERSE.
//
// Both evaluate a cell from the cells it sends flow TO (its at most two downslope receivers), so the sweep starts at the cells
// without receivers and runs upstream; the reference does it with one queue per MPI rank and a share() per outer round.  A
// cell's value depends only on its receivers' values (folded in k = 1..8 order, the reference's order of float32 / float64
// operations), so the tile dependency sweep of d8_sweep.hpp applies with the roles swapped:
//   dependency mask  = the cell's own receivers: prop(angle, k) > 0, inside the raster, with an angle (src/DinfRevAccum.cpp:141-150)
//   release mask     = the neighbours that send flow to the cell (src/DinfRevAccum.cpp:201-219)
// DinfRevAccum's two results travel as one 8-byte record (one store: see d8_sweep.hpp).  The two proportions of a cell are
// recomputed from its angle when it is evaluated (prop() of dinf_prop.hpp: fp64 divisions, per-row atan2 from the host libm).
#include <cmath>
#include <cstring>
#include <vector>

#include "context.hpp"
#include "d8_sweep.hpp"
#include "device_common.hpp"
#include "dinf_prop.hpp"
#include "dinf_rev.hpp"

namespace {
using namespace tdxk;
using namespace dinfrev;

struct UpDepAlg {   // src/DinfUpDependence.cpp:184-208
    using Cell = float;
    using Aux = float2;                          // {angle, disturbance grid value (int bits)}
    static constexpr bool HAS_AUX = true, HAS_DIST = false, HAS_ROWS = true;
    static constexpr int kBulkSweeps = 0;            // (not used: the reverse sweeps run d8sweep::sweep_tile_rev, lockstep sweeps to the end of every activation)
    static constexpr int kMinWaves32 = 5;
    static constexpr int kMaxRelease = 8;
    static constexpr unsigned kBulkUntil = 64;       // a wide front of thousands of tiles to the very end: several small tiles per CU beat one large one (489 -> 380 ms at 16384^2)
    static __device__ __forceinline__ float head(float c) { return c; }
    static __host__ __device__ __forceinline__ float outside() { return -1.0f; }
    static __device__ __forceinline__ unsigned rel_mask(unsigned inf) { return (inf >> 16) & 0xFFu; }
    static __device__ __forceinline__ void rev_row(unsigned inf, const Aux& a, double a2, int (&k)[2], bool (&on)[2], double (&p)[2]) { rev_row_dinf(inf, a.x, a2, k, on, p); }
    __device__ __forceinline__ Cell eval2(const Aux& a, const bool (&on)[2], const double (&p)[2], const Cell (&n)[2]) const {
        if (__float_as_int(a.y) >= 1) return 1.0f;
        float dep = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; t++)
            if (on[t]) dep = dep + (float)(n[t] * p[t]);
        return dep;
    }
    template <class L>
    __device__ __forceinline__ void eval(L& S, int c, int cl, int ly, unsigned inf, const Cell (&nb)[9]) const {
        const float2 a = S.aux[c];
        float dep;
        if (__float_as_int(a.y) >= 1) dep = 1.0f;
        else {
            dep = 0.0f;
            const Recv r = receivers(inf);
#pragma unroll
            for (int t = 0; t < 2; t++) {
                if (!r.on[t] || !((inf >> (r.k[t] - 1)) & 1u)) continue;   // prop > 0, inside the raster, with an angle
                const double p = prop_dev(a.x, r.k[t], S.rows[ly + 1]);
                float depp = 0.f;
#pragma unroll
                for (int k = 1; k <= 8; k++) if (k == r.k[t]) depp = nb[k];
                dep = dep + (float)(depp * p);
            }
        }
        S.v[cl] = dep;
    }
};

struct RevAccAlg {   // src/DinfRevAccum.cpp:176-199; record = {racc, dmax}
    using Cell = float2;
    using Aux = float2;                          // {angle, weight}
    static constexpr bool HAS_AUX = true, HAS_DIST = false, HAS_ROWS = true;
    static constexpr int kBulkSweeps = 0;            // (not used: the reverse sweeps run d8sweep::sweep_tile_rev, lockstep sweeps to the end of every activation)
    static constexpr unsigned kBulkUntil = 64;
    static constexpr int kMinWaves32 = 4;
    static constexpr int kMaxRelease = 8;
    float w_nodata;
    static __device__ __forceinline__ float head(const float2& c) { return c.x; }
    static __host__ __device__ __forceinline__ float2 outside() { return make_float2(TDX_ANG_NODATA, TDX_ANG_NODATA); }
    static __device__ __forceinline__ unsigned rel_mask(unsigned inf) { return (inf >> 16) & 0xFFu; }
    static __device__ __forceinline__ void rev_row(unsigned inf, const Aux& a, double a2, int (&k)[2], bool (&on)[2], double (&p)[2]) { rev_row_dinf(inf, a.x, a2, k, on, p); }
    __device__ __forceinline__ Cell eval2(const Aux& a, const bool (&on)[2], const double (&p)[2], const Cell (&n)[2]) const {
        if (is_nodata_f(a.y, w_nodata)) return make_float2(TDX_ANG_NODATA, TDX_ANG_NODATA);
        float racc = a.y, dmax = a.y;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (!on[t] || is_nodata_f(n[t].x, TDX_ANG_NODATA)) continue;   // (a receiver whose weight was nodata)
            const float valn = (float)(p[t] * n[t].x);
            racc = racc + valn;
            if (n[t].y > dmax) dmax = n[t].y;
        }
        return make_float2(racc, dmax);
    }
    template <class L>
    __device__ __forceinline__ void eval(L& S, int c, int cl, int ly, unsigned inf, const Cell (&nb)[9]) const {
        const float2 a = S.aux[c];
        float racc, dmax;
        if (is_nodata_f(a.y, w_nodata)) { racc = TDX_ANG_NODATA; dmax = TDX_ANG_NODATA; }
        else {
            racc = a.y; dmax = a.y;
            const Recv r = receivers(inf);
#pragma unroll
            for (int t = 0; t < 2; t++) {
                if (!r.on[t] || !((inf >> (r.k[t] - 1)) & 1u)) continue;
                float2 n = make_float2(0.f, 0.f);
#pragma unroll
                for (int k = 1; k <= 8; k++) if (k == r.k[t]) n = nb[k];
                if (is_nodata_f(n.x, TDX_ANG_NODATA)) continue;        // a receiver whose weight was nodata
                const double p = prop_dev(a.x, r.k[t], S.rows[ly + 1]);
                const float valn = (float)(p * n.x);
                racc = racc + valn;
                if (n.y > dmax) dmax = n.y;
            }
        }
        S.v[cl] = make_float2(racc, dmax);
    }
};

__global__ __launch_bounds__(256) void pack_aux_i_kernel(const float* __restrict__ ANG, const int32_t* __restrict__ DG, size_t n, float2* __restrict__ aux) {
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) aux[i] = make_float2(ANG[i], __int_as_float(DG[i]));
}
__global__ __launch_bounds__(256) void pack_aux_f_kernel(const float* __restrict__ ANG, const float* __restrict__ W, size_t n, float2* __restrict__ aux) {
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) aux[i] = make_float2(ANG[i], W[i]);
}
int updep_impl(tdx_context* ctx, const Strip& st, float* d_ang, float ang_nodata, const double* dxc, const double* dyc, int32_t* d_dg, float* d_dep, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t n = size_t(st.nx) * size_t(st.ny_arr);
    const size_t first = size_t(st.y0) * size_t(st.nx), nown = size_t(st.y1 - st.y0) * size_t(st.nx);
    RevSetup R;
    int rc = rev_prepare(ctx, st, d_ang, ang_nodata, dxc, dyc, R, stats);
    if (rc != TDX_OK) return rc;
    hipLaunchKernelGGL(pack_aux_i_kernel, dim3(tdx_blocks_for(n, 256)), dim3(256), 0, s, d_ang, d_dg, n, R.aux);
    hipLaunchKernelGGL(d8sweep::init_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.info, d_dep, first, nown, -1.0f);   // depNodata = -1 (src/DinfUpDependence.cpp:113)
    rc = strip_exchange<float>(ctx, st, d_dep, -1.0f);
    if (rc != TDX_OK) return rc;
    int64_t rounds = 0, launches = 0, outer = 1;
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        d8sweep::Arrays<UpDepAlg> A{d_dep, R.aux, nullptr, R.d_a2, R.info};
        rc = d8sweep::run(ctx, st, UpDepAlg{}, A, R.counts, &rounds, &launches, &outer);
        if (rc != TDX_OK) return rc;
        hipLaunchKernelGGL(d8sweep::finish_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, d_dep, first, nown, -1.0f);
        if (stats) stats->launches[TDX_K_ACCUM] += launches;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    return TDX_OK;
}

int revacc_impl(tdx_context* ctx, const Strip& st, float* d_ang, float ang_nodata, const double* dxc, const double* dyc, float* d_w, float w_nodata, float* d_racc,
                float* d_dmax, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t n = size_t(st.nx) * size_t(st.ny_arr);
    const size_t first = size_t(st.y0) * size_t(st.nx), nown = size_t(st.y1 - st.y0) * size_t(st.nx);
    RevSetup R;
    int rc = rev_prepare(ctx, st, d_ang, ang_nodata, dxc, dyc, R, stats);
    if (rc != TDX_OK) return rc;
    float2* rec = static_cast<float2*>(ctx->scratch(TDX_S_C, n * 8));
    if (!rec) return TDX_ERR_NOMEM;
    hipLaunchKernelGGL(pack_aux_f_kernel, dim3(tdx_blocks_for(n, 256)), dim3(256), 0, s, d_ang, d_w, n, R.aux);
    hipLaunchKernelGGL(rev_init2_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.info, rec, first, nown);
    {
        const float2 oc = RevAccAlg::outside();
        uint2 ob;
        memcpy(&ob, &oc, sizeof(ob));
        rc = strip_exchange<uint2>(ctx, st, reinterpret_cast<uint2*>(rec), ob);
        if (rc != TDX_OK) return rc;
    }
    int64_t rounds = 0, launches = 0, outer = 1;
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        d8sweep::Arrays<RevAccAlg> A{rec, R.aux, nullptr, R.d_a2, R.info};
        rc = d8sweep::run(ctx, st, RevAccAlg{w_nodata}, A, R.counts, &rounds, &launches, &outer);
        if (rc != TDX_OK) return rc;
        hipLaunchKernelGGL(rev_unpack2_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, rec, first, nown, d_racc, d_dmax);
        if (stats) stats->launches[TDX_K_ACCUM] += launches;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    return TDX_OK;
}


}  // namespace

// the argument tests of the _dev (halo 0) and _strip (halo 2: the strip's two halo rows) entry points
static int updep_check(tdx_context* ctx, const void* ang, const void* dg, const void* dep, const void* dxc, const void* dyc, int64_t nx, int64_t ny, int64_t halo,
                       const char* who) {
    if (!ctx || !ang || !dg || !dep || !dxc || !dyc || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}
static int revacc_check(tdx_context* ctx, const void* ang, const void* w, const void* racc, const void* dmax, const void* dxc, const void* dyc, int64_t nx, int64_t ny,
                        int64_t halo, const char* who) {
    if (!ctx || !ang || !w || !racc || !dmax || !dxc || !dyc || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}

extern "C" int tdx_dinfupdependence_dev(tdx_context* ctx, const float* d_ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc,
                                        const int32_t* d_dg, float* d_dep, tdx_stats* stats) {
    if (int rc = updep_check(ctx, d_ang, d_dg, d_dep, dxc, dyc, nx, ny, 0, "tdx_dinfupdependence_dev: bad argument")) return rc;
    return updep_impl(ctx, strip_single(int(nx), int(ny)), const_cast<float*>(d_ang), ang_nodata, dxc, dyc, const_cast<int32_t*>(d_dg), d_dep, stats);
}
extern "C" int tdx_dinfupdependence_strip(tdx_context* ctx, const tdx_comm* comm, float* d_ang, int64_t nx, int64_t ny_local, float ang_nodata, const double* dxc,
                                          const double* dyc, int32_t* d_dg, float* d_dep, tdx_stats* stats) {
    if (int rc = updep_check(ctx, d_ang, d_dg, d_dep, dxc, dyc, nx, ny_local, 2, "tdx_dinfupdependence_strip: bad argument")) return rc;
    return updep_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_ang, ang_nodata, dxc, dyc, d_dg, d_dep, stats);
}
extern "C" int tdx_dinfupdependence(tdx_context* ctx, const float* ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc,
                                    const int32_t* dg, float* dep, tdx_stats* stats) {
    if (!ctx || !ang || !dg || !dep || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_dinfupdependence: bad argument");
    HostCall h(ctx, nx, ny);
    float* d_a = h.in(TDX_S_IO0, ang);
    int32_t* d_g = h.in(TDX_S_IO1, dg);
    float* d_o = h.out(TDX_S_IO2, dep);
    if (h.error) return h.error;
    return h.finish(tdx_dinfupdependence_dev(ctx, d_a, nx, ny, ang_nodata, dxc, dyc, d_g, d_o, stats));
}

extern "C" int tdx_dinfrevaccum_dev(tdx_context* ctx, const float* d_ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc,
                                    const float* d_w, float w_nodata, float* d_racc, float* d_dmax, tdx_stats* stats) {
    if (int rc = revacc_check(ctx, d_ang, d_w, d_racc, d_dmax, dxc, dyc, nx, ny, 0, "tdx_dinfrevaccum_dev: bad argument")) return rc;
    return revacc_impl(ctx, strip_single(int(nx), int(ny)), const_cast<float*>(d_ang), ang_nodata, dxc, dyc, const_cast<float*>(d_w), w_nodata, d_racc, d_dmax, stats);
}
extern "C" int tdx_dinfrevaccum_strip(tdx_context* ctx, const tdx_comm* comm, float* d_ang, int64_t nx, int64_t ny_local, float ang_nodata, const double* dxc,
                                      const double* dyc, float* d_w, float w_nodata, float* d_racc, float* d_dmax, tdx_stats* stats) {
    if (int rc = revacc_check(ctx, d_ang, d_w, d_racc, d_dmax, dxc, dyc, nx, ny_local, 2, "tdx_dinfrevaccum_strip: bad argument")) return rc;
    return revacc_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_ang, ang_nodata, dxc, dyc, d_w, w_nodata, d_racc, d_dmax, stats);
}
extern "C" int tdx_dinfrevaccum(tdx_context* ctx, const float* ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc, const float* w,
                                float w_nodata, float* racc, float* dmax, tdx_stats* stats) {
    if (!ctx || !ang || !w || !racc || !dmax || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_dinfrevaccum: bad argument");
    HostCall h(ctx, nx, ny);
    float* d_a = h.in(TDX_S_IO0, ang);
    float* d_w = h.in(TDX_S_IO1, w);
    float* d_r = h.out(TDX_S_IO2, racc);
    float* d_m = h.out(TDX_S_IO3, dmax);
    if (h.error) return h.error;
    return h.finish(tdx_dinfrevaccum_dev(ctx, d_a, nx, ny, ang_nodata, dxc, dyc, d_w, w_nodata, d_r, d_m, stats));
}
