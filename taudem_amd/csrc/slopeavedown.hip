// SlopeAveDown (sloped, src/SlopeAveDown.cpp:59-330) on gfx950: the slope from each cell to the cell that lies the distance dn down its
// D8 flow path.
//
// The reference runs niter = int(dn / min(dxA, dyA)) + 1 full Kahn passes (initNeighborD8up, src/commonLib.cpp:251-282).  A pass visits
// the cells its queue reaches - the POPPED set, the same in every pass - and each of them with a code 1..8 whose receiver n lies on the
// raster and has ed(n) not nodata does (src/SlopeAveDown.cpp:229-249)
//     ddi = dist[row][p] + dd(n);  zi = ed(n);  if (sd is nodata && ddi > dn) sd = (z - zi) / ddi;  ed = zi;  dd = ddi;
// A receiver is popped after its contributors, so every cell reads what its receiver held at the END OF THE PREVIOUS pass: a pass is a
// Jacobi step, independent of the visiting order and of the rank count.  Here:
//   1. the popped set: one unit-weight run of the forward D8 sweep (d8sweep::SumMaxMin without the contamination check: its result is a
//      count >= 1 exactly on the cells the queue reaches), packed into one byte per cell - the code 1..8 of a popped cell, else 0;
//   2. niter pull passes over two record arrays in turn.  {ed, dd} is ONE 8-byte record, read and written with one instruction (the rule
//      d8_sweep.hpp states for records).  A pass reads the cell's byte and record, gathers its receiver's record (a neighbour: the same
//      or an adjacent cache line), writes the cell's new record, and touches sd (and z) only where ddi > dn.  No atomics, no LDS;
//   3. on strips the halo rows of the record array are exchanged after every pass.
// dist[row][k] is made on the host in double and rounded to float as in d8_rev.hpp.  The sum is nested from the far end (dist_i + (dist_n
// + ...)) because each pass adds the cell's own step to its receiver's finished sum; the division is IEEE (hipcc's default for `/`).
// ed / dd start as z / 0 where z and p are both not nodata, nodata elsewhere: a popped cell with nodata z but a valid code acquires a
// record in the first pass, is seen by its contributors from the second, and its z enters the slope as the nodata VALUE.
#include <algorithm>
#include <cmath>
#include <vector>

#include "context.hpp"
#include "d8_sweep.hpp"
#include "device_common.hpp"

namespace {
using namespace tdxk;

// owned rows: the code byte, the first record and sd.  `pop` is the swept unit-weight count: >= 1 on popped cells, -1 on cells that do
// not take part, the pending pattern (a NaN) on cells the queue never reaches.
__global__ __launch_bounds__(256) void sad_init_kernel(const int16_t* __restrict__ P, int16_t p_nodata, const float* __restrict__ z, float z_nodata,
                                                       const float* __restrict__ pop, size_t first, size_t n, uint8_t* __restrict__ code, float2* __restrict__ rec,
                                                       float* __restrict__ sd) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    const int16_t p = P[i];
    const float zz = z[i];
    code[i] = (pop[i] >= 1.0f && p >= 1 && p <= 8) ? uint8_t(p) : uint8_t(0);
    const bool both = !is_nodata_f(zz, z_nodata) && !is_nodata_s(p, p_nodata);   // src/SlopeAveDown.cpp:157-161
    rec[i] = both ? make_float2(zz, 0.0f) : make_float2(TDX_ANG_NODATA, TDX_ANG_NODATA);
    sd[i] = TDX_ANG_NODATA;
}

// one pass over the owned rows [y0, y0 + rows); a block is 256 consecutive cells of one row.  Receivers are read in array rows
// [row_lo, row_hi): the owned rows and the halo rows a neighbouring rank owns (hasAccess, src/SlopeAveDown.cpp:234).
__global__ __launch_bounds__(256) void sad_pull_kernel(const float2* __restrict__ in, float2* __restrict__ out, const uint8_t* __restrict__ code,
                                                       const float* __restrict__ z, const float* __restrict__ dist, float* __restrict__ sd, double dn, int nx,
                                                       int y0, unsigned blocks_x, int row_lo, int row_hi) {
    const unsigned by = blockIdx.x / blocks_x;
    const int x = int(blockIdx.x - by * blocks_x) * 256 + int(threadIdx.x), y = y0 + int(by);
    if (x >= nx) return;
    const size_t idx = size_t(y) * size_t(nx) + size_t(x);
    const int k = code[idx];
    float2 r = in[idx];
    if (k) {
        const int xn = x + d1(k), yn = y + d2(k);
        if (xn >= 0 && xn < nx && yn >= row_lo && yn < row_hi) {
            const float2 rn = in[size_t(yn) * size_t(nx) + size_t(xn)];
            if (!is_nodata_f(rn.x, TDX_ANG_NODATA)) {
                const float ddi = dist[size_t(y) * 9 + size_t(k)] + rn.y;
                if (double(ddi) > dn && is_nodata_f(sd[idx], TDX_ANG_NODATA)) sd[idx] = (z[idx] - rn.x) / ddi;
                r = make_float2(rn.x, ddi);
            }
        }
    }
    out[idx] = r;
}

int sad_impl(tdx_context* ctx, const Strip& st, int16_t* d_p, int16_t p_nodata, const float* d_z, float z_nodata, const double* dxc, const double* dyc, double dn,
             int64_t niter, float* d_sd, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int inx = st.nx, iny = st.ny_arr;
    const size_t n = size_t(inx) * size_t(iny);
    const size_t first = size_t(st.y0) * size_t(inx), nown = size_t(st.y1 - st.y0) * size_t(inx);
    uint32_t* info = static_cast<uint32_t*>(ctx->scratch(TDX_S_A, n * 4));
    float* pop = static_cast<float*>(ctx->scratch(TDX_S_B, n * 4));
    float2* rec[2] = {static_cast<float2*>(ctx->scratch(TDX_S_C, n * 8)), static_cast<float2*>(ctx->scratch(TDX_S_D, n * 8))};
    uint8_t* code = static_cast<uint8_t*>(ctx->scratch(TDX_S_E, n));
    unsigned long long* counts = static_cast<unsigned long long*>(ctx->scratch(TDX_S_M, size_t(tilek::COUNT_RING) * 16));
    // dist[j][k] = sqrt(d1^2 dxc^2 + d2^2 dyc^2) in double, stored as float (src/SlopeAveDown.cpp:119-128)
    static const int hd1[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1}, hd2[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
    std::vector<float> dist(size_t(iny) * 9, 0.f);
    for (int m = 0; m < iny; m++)
        for (int k = 1; k <= 8; k++) dist[size_t(m) * 9 + size_t(k)] = (float)sqrt(hd1[k] * hd1[k] * dxc[m] * dxc[m] + hd2[k] * hd2[k] * dyc[m] * dyc[m]);
    float* d_dist = static_cast<float*>(ctx->scratch(TDX_S_F, dist.size() * sizeof(float)));
    if (!info || !pop || !rec[0] || !rec[1] || !code || !counts || !d_dist) return TDX_ERR_NOMEM;
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_dist, dist.data(), dist.size() * sizeof(float), hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));   // `dist` is a local
    ctx->begin_call(stats);
    strip_mark(ctx, st, "slopeavedown");
    int rc = strip_exchange<int16_t>(ctx, st, d_p, p_nodata);   // p->share()
    if (rc != TDX_OK) return rc;
    // ---- 1. the popped set
    {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        hipLaunchKernelGGL(d8sweep::setup_kernel, dim3((inx + 63) / 64, (iny + 3) / 4), dim3(256), 0, s, d_p, inx, iny, p_nodata, 0, nullptr, 0, nullptr, info);
        hipLaunchKernelGGL(d8sweep::init_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, info, pop, first, nown, TDX_AREA_NODATA);
        if (stats) stats->launches[TDX_K_STENCIL] += 2;
    }
    rc = strip_exchange<float>(ctx, st, pop, TDX_AREA_NODATA);
    if (rc != TDX_OK) return rc;
    int64_t rounds = 0, launches = 0, outer = 1;
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        d8sweep::SumMaxMin alg{0, TDX_AREA_NODATA, 0.f, 0, false};
        d8sweep::Arrays<d8sweep::SumMaxMin> A{pop, nullptr, nullptr, nullptr, info};
        rc = d8sweep::run(ctx, st, alg, A, counts, &rounds, &launches, &outer);
        if (rc != TDX_OK) return rc;
        if (stats) stats->launches[TDX_K_ACCUM] += launches;
    }
    // ---- 2. the pull passes
    {
        TdxSpan sp(ctx, TDX_K_MISC);
        hipLaunchKernelGGL(sad_init_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, d_p, p_nodata, d_z, z_nodata, pop, first, nown, code, rec[0], d_sd);
        const uint2 nd2 = make_uint2(__builtin_bit_cast(uint32_t, TDX_ANG_NODATA), __builtin_bit_cast(uint32_t, TDX_ANG_NODATA));
        rc = strip_exchange<uint2>(ctx, st, reinterpret_cast<uint2*>(rec[0]), nd2);   // ed->share(), dd->share()
        if (rc != TDX_OK) return rc;
        const unsigned blocks_x = tdx_blocks_for(uint64_t(inx), 256);
        const uint64_t nblocks = uint64_t(blocks_x) * uint64_t(st.y1 - st.y0);
        if (nblocks > 0x7fffffffull) return tdx_fail(ctx, TDX_ERR_ARG, "slopeavedown: strip too large for one launch");
        const int row_lo = st.up ? 0 : st.y0, row_hi = st.down ? iny : st.y1;
        int cur = 0;
        for (int64_t it = 0; it < niter; it++) {
            hipLaunchKernelGGL(sad_pull_kernel, dim3(unsigned(nblocks)), dim3(256), 0, s, rec[cur], rec[cur ^ 1], code, d_z, d_dist, d_sd, dn, inx, st.y0, blocks_x, row_lo,
                               row_hi);
            cur ^= 1;
            if (st.multi()) {
                rc = strip_exchange<uint2>(ctx, st, reinterpret_cast<uint2*>(rec[cur]), nd2);
                if (rc != TDX_OK) return rc;
            }
        }
        if (stats) stats->launches[TDX_K_MISC] += niter + 1;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = niter; stt->cells_evaluated = rounds; }
    return TDX_OK;
}

inline bool bad_dn(double dn) { return !std::isfinite(dn) || dn < 0.0; }

}  // namespace

// niter = int(dn / min(dxA, dyA)) + 1 with the cell sizes of the raster's middle row (tiffIO's dxA / dyA: src/tiffIO.cpp:155-156, src/SlopeAveDown.cpp:172)
extern "C" int64_t tdx_slopeavedown_niter(double dn, const double* dxc, const double* dyc, int64_t ny) {
    if (!dxc || !dyc || ny <= 0 || bad_dn(dn)) return -1;
    const double m = std::min(std::fabs(dxc[ny / 2]), std::fabs(dyc[ny / 2]));
    const double q = dn / m + 1.0;
    if (!(q >= 1.0) || q >= 9.0e18) return -1;   // a zero or NaN cell size
    return int64_t(q);
}

// the argument test of the _dev and _strip entry points, up to where the two part: a strip cannot derive niter
static int sad_check(tdx_context* ctx, const void* p, const void* fel, const void* slpd, const void* dxc, const void* dyc, int64_t nx, int64_t ny, double dn, const char* who) {
    if (!ctx || !p || !fel || !slpd || !dxc || !dyc || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, who);
    return bad_dn(dn) ? tdx_fail(ctx, TDX_ERR_ARG, "slopeavedown: dn must be finite and not negative") : TDX_OK;
}

extern "C" int tdx_slopeavedown_dev(tdx_context* ctx, const int16_t* d_p, int64_t nx, int64_t ny, int16_t p_nodata, const float* d_fel, float fel_nodata,
                                    const double* dxc, const double* dyc, double dn, int64_t niter, float* d_slpd, tdx_stats* stats) {
    if (int rc = sad_check(ctx, d_p, d_fel, d_slpd, dxc, dyc, nx, ny, dn, "tdx_slopeavedown_dev: bad argument")) return rc;
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    if (niter <= 0) niter = tdx_slopeavedown_niter(dn, dxc, dyc, ny);
    if (niter <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "slopeavedown: the cell sizes give no iteration count");
    return sad_impl(ctx, strip_single(int(nx), int(ny)), const_cast<int16_t*>(d_p), p_nodata, d_fel, fel_nodata, dxc, dyc, dn, niter, d_slpd, stats);
}
extern "C" int tdx_slopeavedown_strip(tdx_context* ctx, const tdx_comm* comm, int16_t* d_p, int64_t nx, int64_t ny_local, int16_t p_nodata, const float* d_fel,
                                      float fel_nodata, const double* dxc, const double* dyc, double dn, int64_t niter, float* d_slpd, tdx_stats* stats) {
    if (int rc = sad_check(ctx, d_p, d_fel, d_slpd, dxc, dyc, nx, ny_local, dn, "tdx_slopeavedown_strip: bad argument")) return rc;
    if (niter <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_slopeavedown_strip: niter must be given (a strip does not know the raster's middle row)");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    return sad_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_p, p_nodata, d_fel, fel_nodata, dxc, dyc, dn, niter, d_slpd, stats);
}
extern "C" int tdx_slopeavedown(tdx_context* ctx, const int16_t* p, int64_t nx, int64_t ny, int16_t p_nodata, const float* fel, float fel_nodata, const double* dxc,
                                const double* dyc, double dn, int64_t niter, float* slpd, tdx_stats* stats) {
    if (!ctx || !p || !fel || !slpd || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_slopeavedown: bad argument");
    HostCall h(ctx, nx, ny);
    int16_t* d_p = h.in(TDX_S_IO0, p);
    float* d_o = h.out(TDX_S_IO1, slpd);
    float* d_z = h.in(TDX_S_IO2, fel);
    if (h.error) return h.error;
    return h.finish(tdx_slopeavedown_dev(ctx, d_p, nx, ny, p_nodata, d_z, fel_nodata, dxc, dyc, dn, niter, d_o, stats));
}
