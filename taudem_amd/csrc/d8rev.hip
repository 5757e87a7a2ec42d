// D8HDistToStrm (distgrid, src/D8HDistToStrm.cpp:57-260), D8VDistToStrm (d8vdistdown, src/D8VDistToStrm.cpp:58-276) and GageWatershed (gagewatershed, src/gagewatershed.cpp:56-360) on gfx950: the
// D8 tools that sweep the D8 dependency graph in REVERSE.
//
// Both are a Kahn queue in the reference that starts at the sources (stream cells / gauges) and walks upstream: a cell's value comes
// from the one cell it drains to.  That is the shape of d8sweep::sweep_tile_rev with the set-up of d8_rev.hpp:
//   dependency mask = the cell's receiver (its D8 code 1..8), release mask = the neighbours that drain into it.
// Only one receiver slot is ever on and no proportion is used.
//   D8DistAlg: a float record.  Stream cells evaluate to 0; any other cell to (float)(dist[j][p] + its receiver's distance), nodata
//     where the receiver's is (src/D8HDistToStrm.cpp:171-180).  The step dist[j][p] is the cell's own input record (made by the set-up),
//     so an evaluation is one float add.  D8VDistToStrm is the same policy with the step fel - fel(receiver) (float, no nodata test:
//     src/D8VDistToStrm.cpp:191-198).  Cells never released - draining off the raster, into a nodata cell that is not a stream
//     cell, around a cycle - finish as nodata, as in the reference.
//   GageAlg: an int32 record that carries the INDEX of the outlet (0 .. n - 1) whose gauge labels the cell, mapped to the user's id
//     when the result is unpacked (an arbitrary id could collide with the pending pattern).  Gauges are seeded and never evaluated; a
//     cell with p 1..8 takes its receiver's label (src/gagewatershed.cpp:226-233); everything unreached is MISSINGLONG.
// GageWatershed's `-id` table comes from the final labels: the gauge G of a placed outlet whose downstream neighbour D lies in the raster
// and is labelled has iddown = label(D) (src/gagewatershed.cpp:259-284, reduced with MAX over the ranks: :322).  On strips D may lie in
// the halo row: d8sweep::run ends with an exchange that found nothing new, so the halo rows hold the neighbours' final labels.
#include <algorithm>
#include <cstring>
#include <unordered_set>
#include <vector>

#include "context.hpp"
#include "d8_rev.hpp"
#include "d8_sweep.hpp"
#include "device_common.hpp"

namespace {
using namespace tdxk;
using namespace d8rev;

struct D8DistAlg {   // src/D8HDistToStrm.cpp:166-180
    using Cell = float;
    using Aux = float;                              // the cell's own step: dist[j][p]; 0 on stream cells; nodata without a receiver
    static constexpr bool HAS_AUX = true, HAS_DIST = false, HAS_ROWS = false;
    static constexpr int kBulkSweeps = 0;            // (not used by sweep_tile_rev)
    static constexpr unsigned kBulkUntil = 64;
    static constexpr int kMinWaves32 = 5;
    static constexpr int kMaxRelease = 8;
    static __device__ __forceinline__ float head(float c) { return c; }
    static __host__ __device__ __forceinline__ float outside() { return TDX_ANG_NODATA; }
    static __device__ __forceinline__ unsigned rel_mask(unsigned inf) { return (inf >> 16) & 0xFFu; }
    static __device__ __forceinline__ void rev_row(unsigned inf, const Aux&, double, int (&k)[2], bool (&on)[2], double (&p)[2]) { rev_row_d8(inf, k, on, p); }
    __device__ __forceinline__ Cell eval2(const Aux& a, const bool (&on)[2], const double (&)[2], const Cell (&n)[2]) const {
        if (!on[0]) return a;                                            // stream cell (0) or no receiver (nodata)
        return is_nodata_f(n[0], TDX_ANG_NODATA) ? TDX_ANG_NODATA : a + n[0];
    }
    template <class L>
    __device__ __forceinline__ void eval(L& S, int c, int cl, int, unsigned inf, const Cell (&nb)[9]) const {
        int k[2];
        bool on[2];
        double p[2];
        rev_row_d8(inf, k, on, p);
        Cell n[2] = {0.f, 0.f};
#pragma unroll
        for (int kk = 1; kk <= 8; kk++) if (kk == k[0]) n[0] = nb[kk];
        S.v[cl] = eval2(S.aux[c], on, p, n);
    }
};

__global__ __launch_bounds__(256) void gw_init_kernel(const uint32_t* __restrict__ info, int32_t* __restrict__ rec, size_t first, size_t n) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < first + n) rec[i] = (info[i] & d8sweep::INFO_PART) ? int32_t(d8sweep::PENDING_BITS) : GW_NODATA;
}
// gauges: their outlet's index, and no dependency (a gauge is never evaluated; not a participating cell for the verifier either)
__global__ __launch_bounds__(256) void gw_seed_kernel(const uint32_t* __restrict__ cell, const int32_t* __restrict__ outlet, int nseed, uint32_t* __restrict__ info,
                                                      int32_t* __restrict__ rec) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nseed) return;
    const size_t c = cell[s];
    rec[c] = outlet[s];
    info[c] &= ~(d8sweep::INFO_PART | 0xFFu);
}
// the outlet index of the label of each gauge's downstream neighbour, or -1 (src/gagewatershed.cpp:257-284): the gauge's code is 1..8, the
// neighbour lies in the raster (rows of the array that are owned or a neighbouring rank's halo) and is labelled
__global__ __launch_bounds__(256) void gw_down_kernel(const uint32_t* __restrict__ cell, int nseed, const int16_t* __restrict__ P, int16_t nodata, const int32_t* __restrict__ rec,
                                                      int nx, int row_lo, int row_hi, int nout, int32_t* __restrict__ down) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nseed) return;
    const size_t c = cell[s];
    const int x = int(c % size_t(nx)), y = int(c / size_t(nx));
    const int16_t p = P[c];
    int32_t d = -1;
    if (!is_nodata_s(p, nodata) && p >= 1 && p <= 8) {
        const int xd = x + d1(p), yd = y + d2(p);
        if (xd >= 0 && xd < nx && yd >= row_lo && yd < row_hi) {
            const int32_t lab = rec[size_t(yd) * size_t(nx) + size_t(xd)];
            if (!d8sweep::pending(__int_as_float(lab)) && lab >= 0 && lab < nout) d = lab;
        }
    }
    down[s] = d;
}
// outlet index -> the user's id; still pending (on or above a cycle) or unreached: MISSINGLONG
__global__ __launch_bounds__(256) void gw_unpack_kernel(int32_t* __restrict__ rec, size_t first, size_t n, const int32_t* __restrict__ ids, int nout) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    const int32_t v = rec[i];
    rec[i] = (!d8sweep::pending(__int_as_float(v)) && v >= 0 && v < nout) ? ids[v] : GW_NODATA;
}

// d_fel != nullptr: D8VDistToStrm (the step is the drop to the receiver; dxc / dyc are not used), else D8HDistToStrm
int d8dist_impl(tdx_context* ctx, const Strip& st, int16_t* d_p, int16_t p_nodata, const int32_t* d_src, int32_t src_nodata, int32_t thresh, const double* dxc,
                const double* dyc, float* d_dist, tdx_stats* stats, float* d_fel = nullptr) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t n = size_t(st.nx) * size_t(st.ny_arr);
    const size_t first = size_t(st.y0) * size_t(st.nx), nown = size_t(st.y1 - st.y0) * size_t(st.nx);
    float* step = static_cast<float*>(ctx->scratch(TDX_S_B, n * 4));
    if (!step) return TDX_ERR_NOMEM;
    RevSetup R;
    int rc = rev_prepare(ctx, st, d_p, p_nodata, d_fel ? MODE_VDIST : MODE_DIST, d_src, src_nodata, thresh, dxc, dyc, step, R, stats,
                         d_fel ? "d8vdisttostrm" : "d8hdisttostrm", d_fel);
    if (rc != TDX_OK) return rc;
    hipLaunchKernelGGL(d8sweep::init_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.info, d_dist, first, nown, TDX_ANG_NODATA);
    rc = strip_exchange<float>(ctx, st, d_dist, TDX_ANG_NODATA);
    if (rc != TDX_OK) return rc;
    int64_t rounds = 0, launches = 0, outer = 1;
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        d8sweep::Arrays<D8DistAlg> A{d_dist, step, nullptr, nullptr, R.info};
        rc = d8sweep::run(ctx, st, D8DistAlg{}, A, R.counts, &rounds, &launches, &outer);
        if (rc != TDX_OK) return rc;
        hipLaunchKernelGGL(d8sweep::finish_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, d_dist, first, nown, TDX_ANG_NODATA);
        if (stats) stats->launches[TDX_K_ACCUM] += launches;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    return TDX_OK;
}

// outlet_x: global columns; outlet_row: rows of the device array (outside the owned rows: not on this rank).  ids: NULL = index + 1.
// placed / iddown: HOST arrays of n_outlets, the same on every rank (reduced with MAX over the ranks, as the reference does).
int gage_impl(tdx_context* ctx, const Strip& st, int16_t* d_p, int16_t p_nodata, const int32_t* outlet_x, const int32_t* outlet_row, const int32_t* ids_in, int64_t nout,
              int32_t* d_gw, int32_t* placed, int32_t* iddown, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t first = size_t(st.y0) * size_t(st.nx), nown = size_t(st.y1 - st.y0) * size_t(st.nx);
    std::vector<int32_t> ids(static_cast<size_t>(nout));
    for (int64_t i = 0; i < nout; i++) ids[size_t(i)] = ids_in ? ids_in[i] : int32_t(i + 1);
    // placement (src/gagewatershed.cpp:172-191): outlets in the owned rows, the first one on a cell wins
    std::vector<uint32_t> seed_cell;
    std::vector<int32_t> seed_outlet;
    {
        std::unordered_set<uint32_t> taken;
        for (int64_t i = 0; i < nout; i++) {
            const int32_t x = outlet_x[i], y = outlet_row[i];
            if (x < 0 || x >= st.nx || y < st.y0 || y >= st.y1) continue;
            const uint32_t c = uint32_t(size_t(y) * size_t(st.nx) + size_t(x));
            if (!taken.insert(c).second) continue;
            seed_cell.push_back(c);
            seed_outlet.push_back(int32_t(i));
        }
    }
    const int nseed = int(seed_cell.size());
    int32_t* d_buf = static_cast<int32_t*>(ctx->scratch(TDX_S_H, (size_t(nseed) * 3 + size_t(nout) + 1) * 4));   // cells, outlets, down, ids
    if (!d_buf) return TDX_ERR_NOMEM;
    uint32_t* d_cell = reinterpret_cast<uint32_t*>(d_buf);
    int32_t* d_outlet = d_buf + nseed;
    int32_t* d_down = d_buf + 2 * size_t(nseed);
    int32_t* d_ids = d_buf + 3 * size_t(nseed);
    if (nseed) {
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_cell, seed_cell.data(), size_t(nseed) * 4, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_outlet, seed_outlet.data(), size_t(nseed) * 4, hipMemcpyHostToDevice, s));
    }
    if (nout) TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_ids, ids.data(), size_t(nout) * 4, hipMemcpyHostToDevice, s));
    RevSetup R;
    int rc = rev_prepare(ctx, st, d_p, p_nodata, MODE_GAGE, nullptr, 0, 0, nullptr, nullptr, nullptr, R, stats, "gagewatershed");
    if (rc != TDX_OK) return rc;
    hipLaunchKernelGGL(gw_init_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.info, d_gw, first, nown);
    if (nseed) hipLaunchKernelGGL(gw_seed_kernel, dim3((nseed + 255) / 256), dim3(256), 0, s, d_cell, d_outlet, nseed, R.info, d_gw);
    rc = strip_exchange<uint32_t>(ctx, st, reinterpret_cast<uint32_t*>(d_gw), uint32_t(GW_NODATA));
    if (rc != TDX_OK) return rc;
    int64_t rounds = 0, launches = 0, outer = 1;
    std::vector<int32_t> down(static_cast<size_t>(nseed));
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        d8sweep::Arrays<GageAlg> A{d_gw, nullptr, nullptr, nullptr, R.info};
        rc = d8sweep::run(ctx, st, GageAlg{}, A, R.counts, &rounds, &launches, &outer);
        if (rc != TDX_OK) return rc;
        const int row_lo = st.up ? 0 : st.y0, row_hi = st.down ? st.ny_arr : st.y1;   // a halo row counts where a neighbouring rank owns it
        if (nseed) {
            hipLaunchKernelGGL(gw_down_kernel, dim3((nseed + 255) / 256), dim3(256), 0, s, d_cell, nseed, d_p, p_nodata, d_gw, st.nx, row_lo, row_hi, int(nout), d_down);
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(down.data(), d_down, size_t(nseed) * 4, hipMemcpyDeviceToHost, s));
        }
        hipLaunchKernelGGL(gw_unpack_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, d_gw, first, nown, d_ids, int(nout));
        if (stats) stats->launches[TDX_K_ACCUM] += launches;
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    // per outlet: placed on this rank (bit 32) and the outlet index of its downstream label + 1 (bits 0..31); one rank places an outlet, so
    // MAX over the ranks (MPI_Reduce(..., MPI_MAX), src/gagewatershed.cpp:320-322) picks that rank's entry
    std::vector<int64_t> red(static_cast<size_t>(nout), 0);
    for (int i = 0; i < nseed; i++) red[size_t(seed_outlet[size_t(i)])] = (int64_t(1) << 32) | int64_t(down[size_t(i)] + 1);
    for (int64_t o = 0; o < nout; o += 16) {
        rc = strip_allreduce(ctx, st, red.data() + o, int(std::min<int64_t>(16, nout - o)), TDX_OP_MAX);
        if (rc != TDX_OK) return rc;
    }
    // dsids[first index with ids == label(G)] = label(D), -1 elsewhere (src/gagewatershed.cpp:176-190, 274-283)
    for (int64_t i = 0; i < nout; i++) { placed[i] = int32_t(red[size_t(i)] >> 32); iddown[i] = -1; }
    for (int64_t i = 0; i < nout; i++) {
        const int64_t d = (red[size_t(i)] & 0xffffffffll) - 1;
        if (!placed[i] || d < 0) continue;
        int64_t j = 0;
        while (ids[size_t(j)] != ids[size_t(i)]) j++;
        iddown[j] = ids[size_t(d)];   // (one gauge per id: one write; the 1-rank result also for a negative id, which MAX over ranks would lose to -1)
    }
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    return TDX_OK;
}

}  // namespace

// the argument tests of the _dev (halo 0) and _strip (halo 2: the strip's two halo rows) entry points
static int d8hdist_check(tdx_context* ctx, const void* p, const void* src, const void* dist, const void* dxc, const void* dyc, int64_t nx, int64_t ny, int64_t halo,
                         const char* who) {
    if (!ctx || !p || !src || !dist || !dxc || !dyc || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}
static int d8vdist_check(tdx_context* ctx, const void* p, const void* fel, const void* src, const void* dist, int64_t nx, int64_t ny, int64_t halo, const char* who) {
    if (!ctx || !p || !fel || !src || !dist || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}
static int gage_check(tdx_context* ctx, const void* p, const void* gw, int64_t nx, int64_t ny, int64_t halo, const int32_t* outlet_x, const int32_t* outlet_y,
                      int64_t n_outlets, const void* placed, const void* iddown, const char* who) {
    if (!ctx || !p || !gw || nx <= 0 || ny <= 0 || n_outlets < 0 || n_outlets > 0x7ffffffe || (n_outlets > 0 && (!outlet_x || !outlet_y || !placed || !iddown)))
        return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}

extern "C" int tdx_d8hdisttostrm_dev(tdx_context* ctx, const int16_t* d_p, int64_t nx, int64_t ny, int16_t p_nodata, const int32_t* d_src, int32_t src_nodata,
                                     int32_t thresh, const double* dxc, const double* dyc, float* d_dist, tdx_stats* stats) {
    if (int rc = d8hdist_check(ctx, d_p, d_src, d_dist, dxc, dyc, nx, ny, 0, "tdx_d8hdisttostrm_dev: bad argument")) return rc;
    return d8dist_impl(ctx, strip_single(int(nx), int(ny)), const_cast<int16_t*>(d_p), p_nodata, d_src, src_nodata, thresh, dxc, dyc, d_dist, stats);
}
extern "C" int tdx_d8hdisttostrm_strip(tdx_context* ctx, const tdx_comm* comm, int16_t* d_p, int64_t nx, int64_t ny_local, int16_t p_nodata, const int32_t* d_src,
                                       int32_t src_nodata, int32_t thresh, const double* dxc, const double* dyc, float* d_dist, tdx_stats* stats) {
    if (int rc = d8hdist_check(ctx, d_p, d_src, d_dist, dxc, dyc, nx, ny_local, 2, "tdx_d8hdisttostrm_strip: bad argument")) return rc;
    return d8dist_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_p, p_nodata, d_src, src_nodata, thresh, dxc, dyc, d_dist, stats);
}
extern "C" int tdx_d8hdisttostrm(tdx_context* ctx, const int16_t* p, int64_t nx, int64_t ny, int16_t p_nodata, const int32_t* src, int32_t src_nodata, int32_t thresh,
                                 const double* dxc, const double* dyc, float* dist, tdx_stats* stats) {
    if (!ctx || !p || !src || !dist || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_d8hdisttostrm: bad argument");
    HostCall h(ctx, nx, ny);
    int16_t* d_p = h.in(TDX_S_IO0, p);
    int32_t* d_s = h.in(TDX_S_IO1, src);
    float* d_o = h.out(TDX_S_IO2, dist);
    if (h.error) return h.error;
    return h.finish(tdx_d8hdisttostrm_dev(ctx, d_p, nx, ny, p_nodata, d_s, src_nodata, thresh, dxc, dyc, d_o, stats));
}

// D8VDistToStrm (d8vdistdown, src/D8VDistToStrm.cpp:58-276): the same sweep with the drop to the receiver as the step.  fel's halo rows are
// exchanged by the set-up, so the strip form writes them.
extern "C" int tdx_d8vdisttostrm_dev(tdx_context* ctx, const int16_t* d_p, int64_t nx, int64_t ny, int16_t p_nodata, const float* d_fel, const int32_t* d_src,
                                     int32_t src_nodata, int32_t thresh, float* d_dist, tdx_stats* stats) {
    if (int rc = d8vdist_check(ctx, d_p, d_fel, d_src, d_dist, nx, ny, 0, "tdx_d8vdisttostrm_dev: bad argument")) return rc;
    return d8dist_impl(ctx, strip_single(int(nx), int(ny)), const_cast<int16_t*>(d_p), p_nodata, d_src, src_nodata, thresh, nullptr, nullptr, d_dist, stats,
                       const_cast<float*>(d_fel));   // (a single strip has no halo rows: nothing is written)
}
extern "C" int tdx_d8vdisttostrm_strip(tdx_context* ctx, const tdx_comm* comm, int16_t* d_p, int64_t nx, int64_t ny_local, int16_t p_nodata, float* d_fel,
                                       const int32_t* d_src, int32_t src_nodata, int32_t thresh, float* d_dist, tdx_stats* stats) {
    if (int rc = d8vdist_check(ctx, d_p, d_fel, d_src, d_dist, nx, ny_local, 2, "tdx_d8vdisttostrm_strip: bad argument")) return rc;
    return d8dist_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_p, p_nodata, d_src, src_nodata, thresh, nullptr, nullptr, d_dist, stats, d_fel);
}
extern "C" int tdx_d8vdisttostrm(tdx_context* ctx, const int16_t* p, int64_t nx, int64_t ny, int16_t p_nodata, const float* fel, const int32_t* src,
                                 int32_t src_nodata, int32_t thresh, float* dist, tdx_stats* stats) {
    if (!ctx || !p || !fel || !src || !dist || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_d8vdisttostrm: bad argument");
    HostCall h(ctx, nx, ny);
    int16_t* d_p = h.in(TDX_S_IO0, p);
    int32_t* d_s = h.in(TDX_S_IO1, src);
    float* d_o = h.out(TDX_S_IO2, dist);
    float* d_f = h.in(TDX_S_IO3, fel);
    if (h.error) return h.error;
    return h.finish(tdx_d8vdisttostrm_dev(ctx, d_p, nx, ny, p_nodata, d_f, d_s, src_nodata, thresh, d_o, stats));
}

extern "C" int tdx_gagewatershed_dev(tdx_context* ctx, const int16_t* d_p, int64_t nx, int64_t ny, int16_t p_nodata, const int32_t* outlet_x, const int32_t* outlet_y,
                                     const int32_t* ids, int64_t n_outlets, int32_t* d_gw, int32_t* placed, int32_t* iddown, tdx_stats* stats) {
    if (int rc = gage_check(ctx, d_p, d_gw, nx, ny, 0, outlet_x, outlet_y, n_outlets, placed, iddown, "tdx_gagewatershed_dev: bad argument")) return rc;
    return gage_impl(ctx, strip_single(int(nx), int(ny)), const_cast<int16_t*>(d_p), p_nodata, outlet_x, outlet_y, ids, n_outlets, d_gw, placed, iddown, stats);
}
extern "C" int tdx_gagewatershed_strip(tdx_context* ctx, const tdx_comm* comm, int16_t* d_p, int64_t nx, int64_t ny_local, int16_t p_nodata, const int32_t* outlet_x,
                                       const int32_t* outlet_row, const int32_t* ids, int64_t n_outlets, int32_t* d_gw, int32_t* placed, int32_t* iddown,
                                       tdx_stats* stats) {
    if (int rc = gage_check(ctx, d_p, d_gw, nx, ny_local, 2, outlet_x, outlet_row, n_outlets, placed, iddown, "tdx_gagewatershed_strip: bad argument")) return rc;
    return gage_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_p, p_nodata, outlet_x, outlet_row, ids, n_outlets, d_gw, placed, iddown, stats);
}
extern "C" int tdx_gagewatershed(tdx_context* ctx, const int16_t* p, int64_t nx, int64_t ny, int16_t p_nodata, const int32_t* outlet_x, const int32_t* outlet_y,
                                 const int32_t* ids, int64_t n_outlets, int32_t* gw, int32_t* placed, int32_t* iddown, tdx_stats* stats) {
    if (!ctx || !p || !gw || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_gagewatershed: bad argument");
    HostCall h(ctx, nx, ny);
    int16_t* d_p = h.in(TDX_S_IO0, p);
    int32_t* d_o = h.out(TDX_S_IO1, gw);
    if (h.error) return h.error;
    return h.finish(tdx_gagewatershed_dev(ctx, d_p, nx, ny, p_nodata, outlet_x, outlet_y, ids, n_outlets, d_o, placed, iddown, stats));
}
