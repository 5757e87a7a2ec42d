// DropAnalysis (src/DropAnalysis.cpp:172-705): for each of nthresh candidate thresholds the stream mask ssa >= thresh is ordered, the elevation drop of every
// Strahler stream is collected and a t-test compares the first-order drops with the higher-order ones; the smallest threshold with |t| < 2 is the optimum
// that Threshold is then run with.
//
// Per threshold: one forward D8 dependency sweep (d8_sweep.hpp, policy DropAlg: order and elevOut of every mask cell, an 8-byte record) and one streaming
// pass over the FINAL records (da_stats_kernel): every junction re-runs updateAtJunction (src/DropAnalysis.cpp:67-110) from its inflows' records and emits its
// drops, every mask cell counts its inflow links by direction class per row.  p, fel and ssa stay on the device for all thresholds; only the info words are
// rebuilt.  Nothing here depends on the schedule:
//   * n1, n2 and the per-row link counts are integers (integer atomics per row);
//   * the four drop sums are fp64, added in a fixed order: a lane's cells top to bottom, a butterfly over the wave, the four waves through LDS, then the
//     workgroups' partials in workgroup order by da_reduce_kernel - no float atomics, so two runs give the same bits;
//   * the length is formed on the host from the integer counts and the cell sizes, in row order.
// The reference adds the same terms in float, in the order its queue pops them (and in rank order with several ranks): its sums and its length are
// order-dependent and are matched within rounding, not bit for bit.  Exact: the ladder, n1, n2, every drop, order and elevOut of every cell, the total area.
//
// Mask and links (src/DropAnalysis.cpp:421-456, 489-503): a cell is on the mask when its ssa is not nodata and >= thresh; neighbour k feeds it when it is
// inside the raster, has a direction 1..8 that points at the cell and is itself on the mask.  Cells on or below a cycle never become ready and keep the
// pending pattern: they have no record, like the reference's never-queued cells.
#include "context.hpp"
#include "d8_sweep.hpp"
#include "device_common.hpp"
#include "dropan_table.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace {
using namespace tdxk;
using d8sweep::DropAlg;

constexpr int16_t DA_ORDER_NODATA = -32768;          // MISSINGSHORT, src/commonLib.h
constexpr float DA_ELEV_NODATA = -3.402823466e38f;   // MISSINGFLOAT

__device__ __forceinline__ bool da_on_mask(float v, float nodata, float thresh) { return !is_nodata_f(v, nodata) && v >= thresh; }

// info words of one threshold (layout: d8_sweep.hpp).  A cell off the mask gets 0: no record, nobody's contributor.
__global__ __launch_bounds__(256) void da_setup_kernel(const int16_t* __restrict__ P, const float* __restrict__ ssa, int nx, int ny, int16_t p_nodata, float ssa_nodata,
                                                       float thresh, uint32_t* __restrict__ info) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= nx || y >= ny) return;
    const size_t idx = size_t(y) * size_t(nx) + size_t(x);
    unsigned inf = 0;
    if (da_on_mask(ssa[idx], ssa_nodata, thresh)) {
#pragma unroll
        for (int k = 1; k <= 8; k++) {
            const int xn = x + d1(k), yn = y + d2(k);
            if (xn < 0 || xn >= nx || yn < 0 || yn >= ny) continue;
            const size_t n = size_t(yn) * size_t(nx) + size_t(xn);
            const int16_t pn = P[n];
            if (is_nodata_s(pn, p_nodata) || pn < 1 || pn > 8) continue;   // pointsToMe (src/DropAnalysis.cpp:56-64)
            if (!(pn - k == 4 || pn - k == -4)) continue;
            if (da_on_mask(ssa[n], ssa_nodata, thresh)) inf |= (1u << (k - 1)) | (1u << (16 + k - 1));
        }
        const int16_t p = P[idx];
        const unsigned code = (!is_nodata_s(p, p_nodata) && p >= 1 && p <= 8) ? unsigned(p) : 15u;
        inf |= (code << 9) | d8sweep::INFO_PART | d8sweep::INFO_OWNMASK;
    }
    info[idx] = inf;
}

// initial records on the owned rows: pending on the mask, "no record" elsewhere
__global__ __launch_bounds__(256) void da_init_kernel(const uint32_t* __restrict__ info, size_t first, size_t n, float2* __restrict__ rec) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    rec[i] = (info[i] & d8sweep::INFO_PART) ? make_float2(__uint_as_float(d8sweep::PENDING_BITS), 0.f) : DropAlg::outside();
}

struct DaPartial { double s[4]; long long n[2]; };   // s1, s1sq, s2, s2sq, n1, n2

__device__ __forceinline__ double da_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ long long da_wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// the four waves' values through LDS, added by thread 0 in wave order
__device__ __forceinline__ void da_block_store(const double (&s)[4], const long long (&n)[2], DaPartial* __restrict__ out) {
    __shared__ DaPartial sh[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    DaPartial mine;
#pragma unroll
    for (int i = 0; i < 4; i++) mine.s[i] = da_wave_sum(s[i]);
#pragma unroll
    for (int i = 0; i < 2; i++) mine.n[i] = da_wave_sum(n[i]);
    if (lane == 0) sh[w] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        DaPartial t = sh[0];
        for (int v = 1; v < 4; v++) {
            for (int i = 0; i < 4; i++) t.s[i] += sh[v].s[i];
            for (int i = 0; i < 2; i++) t.n[i] += sh[v].n[i];
        }
        *out = t;
    }
}

// One workgroup per 64 x 64 block of the owned rows [y0, y1): wave w takes the block's rows w, w + 4 ..., a lane one column.  rowcnt[3 * row + class]: inflow
// links of the row's cells, class 0 = E-W (m 1 / 5), 1 = N-S (m 3 / 7), 2 = diagonal (src/DropAnalysis.cpp:494-501).
__global__ __launch_bounds__(256) void da_stats_kernel(const float2* __restrict__ rec, const uint32_t* __restrict__ info, const float* __restrict__ fel, int nx, int y0,
                                                       int y1, uint32_t* __restrict__ rowcnt, DaPartial* __restrict__ partial) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane;
    double s[4] = {0., 0., 0., 0.};
    long long n[2] = {0, 0};
    for (int it = 0; it < 16; it++) {
        const int y = y0 + int(blockIdx.y) * 64 + it * 4 + w;   // the same for the whole wave
        unsigned links = 0;   // three 10-bit fields: a cell has at most 2 / 2 / 4 links of a class, a wave 64 cells
        if (x < nx && y < y1) {
            const size_t idx = size_t(y) * size_t(nx) + size_t(x);
            const unsigned inf = info[idx];
            if (inf & d8sweep::INFO_PART) {
                const float2 me = rec[idx];
                if (!d8sweep::pending(me.x)) {
                    const unsigned vmask = (inf >> 16) & 0xFFu;
                    links = unsigned(__popc(vmask & 0x11u)) | (unsigned(__popc(vmask & 0x44u)) << 10) | (unsigned(__popc(vmask & 0xAAu)) << 20);
                    if (__popc(vmask) >= 2) {   // a junction: its inflows are inside the array (da_setup_kernel) and have their final records
                        float2 nb[9];
#pragma unroll
                        for (int k = 1; k <= 8; k++)
                            nb[k] = ((vmask >> (k - 1)) & 1u) ? rec[size_t(y + d2(k)) * size_t(nx) + size_t(x + d1(k))] : DropAlg::outside();
                        int count;
                        float e;
                        const int oOut = DropAlg::order_of(vmask, nb, count, e);
                        const float f = fel[idx];
#pragma unroll
                        for (int k = 1; k <= 8; k++) {
                            if (!((vmask >> (k - 1)) & 1u)) continue;
                            const int o = __float_as_int(nb[k].x);
                            if (o >= oOut) continue;
                            const float drop = nb[k].y - f;        // one float subtraction, as in the reference
                            const float sq = drop * drop;          // ... and its float square
                            const int c = o == 1 ? 0 : 1;
                            s[2 * c] += double(drop);
                            s[2 * c + 1] += double(sq);
                            n[c]++;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) links += __shfl_xor(links, off, 64);
        if (lane == 0 && links != 0u) {
            if (links & 1023u) atomicAdd(&rowcnt[3 * size_t(y) + 0], links & 1023u);
            if ((links >> 10) & 1023u) atomicAdd(&rowcnt[3 * size_t(y) + 1], (links >> 10) & 1023u);
            if (links >> 20) atomicAdd(&rowcnt[3 * size_t(y) + 2], links >> 20);
        }
    }
    da_block_store(s, n, partial + size_t(blockIdx.y) * gridDim.x + blockIdx.x);
}

// the workgroups' partials in workgroup order: thread t adds partials t, t + 256 ..., then the same fixed tree
__global__ __launch_bounds__(256) void da_reduce_kernel(const DaPartial* __restrict__ partial, unsigned nparts, DaPartial* __restrict__ out) {
    double s[4] = {0., 0., 0., 0.};
    long long n[2] = {0, 0};
    for (unsigned b = threadIdx.x; b < nparts; b += 256u) {
        const DaPartial p = partial[b];
        for (int i = 0; i < 4; i++) s[i] += p.s[i];
        for (int i = 0; i < 2; i++) n[i] += p.n[i];
    }
    da_block_store(s, n, out);
}

// Total area (src/DropAnalysis.cpp:304-331), one thread per outlet: flag 0 = not in the owned rows or not terminal, 1 = terminal (term = its ad8),
// 2 = on a cell without a direction 0..8 (the reference indexes outside its offset table there).  Terminal: the downstream neighbour's ssa is nodata
// or <= 0, or the neighbour is outside the raster.
__global__ __launch_bounds__(256) void da_outlet_kernel(const int32_t* __restrict__ ox, const int32_t* __restrict__ oy, int nout, int nx, int ny_arr, int y0, int y1,
                                                        const float* __restrict__ ad8, const int16_t* __restrict__ P, int16_t p_nodata, const float* __restrict__ ssa,
                                                        float ssa_nodata, float* __restrict__ term, int32_t* __restrict__ flag) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= nout) return;
    const int x = ox[o], y = oy[o];
    float t = 0.f;
    int f = 0;
    if (x >= 0 && x < nx && y >= y0 && y < y1) {
        const size_t idx = size_t(y) * size_t(nx) + size_t(x);
        const int16_t p = P[idx];
        if (is_nodata_s(p, p_nodata) || p < 0 || p > 8) f = 2;
        else {
            const int xn = x + d1(p), yn = y + d2(p);
            bool terminal = true;
            if (xn >= 0 && xn < nx && yn >= 0 && yn < ny_arr) {
                const float sv = ssa[size_t(yn) * size_t(nx) + size_t(xn)];
                terminal = is_nodata_f(sv, ssa_nodata) || sv <= 0.f;
            }
            if (terminal) { f = 1; t = ad8[idx]; }
        }
    }
    term[o] = t;
    flag[o] = f;
}

// the records of one threshold as two rasters (the test hook grid_th): no record -> nodata
__global__ __launch_bounds__(256) void da_grids_kernel(const float2* __restrict__ rec, size_t first, size_t n, int16_t* __restrict__ order, float* __restrict__ elev) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    const float2 r = rec[i];
    const int o = __float_as_int(r.x);
    const bool has = !d8sweep::pending(r.x) && o > 0;
    if (order) order[i] = has ? int16_t(o) : DA_ORDER_NODATA;
    if (elev) elev[i] = has ? r.y : DA_ELEV_NODATA;
}

struct DaResult {   // host arrays of the caller
    float* thresh;
    int64_t *n1, *n2;
    double* sums;     // [nthresh][4]: s1, s1sq, s2, s2sq
    double* length;
};

// One strip of dropan().  dxc / dyc: cell sizes of the rows of the strip array.  outlet_term (host, n_outlets floats): ad8 of the outlets of the owned rows that
// are terminal, 0 for every other outlet; the caller adds them in file order.  The strip's own n1 / n2 / sums / length go to `res`.
int dropan_impl(tdx_context* ctx, const Strip& st, const float* d_ad8, int16_t* d_p, int16_t p_nodata, float* d_fel, float* d_ssa, float ssa_nodata, const double* dxc,
                const double* dyc, const int32_t* outlet_x, const int32_t* outlet_y, int64_t n_outlets, float thresh_min, float thresh_max, int64_t nthresh, int steptype,
                int64_t grid_th, int16_t* d_order, float* d_elev, const DaResult& res, float* outlet_term, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int inx = st.nx, iny = st.ny_arr;
    const size_t n = size_t(inx) * size_t(iny);
    const size_t first = size_t(st.y0) * size_t(inx), nown = size_t(st.y1 - st.y0) * size_t(inx);
    const dim3 grid2d((inx + 63) / 64, (iny + 3) / 4);
    const dim3 grid_stats((inx + 63) / 64, (st.y1 - st.y0 + 63) / 64);
    const unsigned nparts = grid_stats.x * grid_stats.y;
    const size_t nout = size_t(n_outlets > 0 ? n_outlets : 0);

    uint32_t* info = static_cast<uint32_t*>(ctx->scratch(TDX_S_A, n * 4));
    float2* rec = static_cast<float2*>(ctx->scratch(TDX_S_C, n * sizeof(float2)));
    unsigned long long* counts = static_cast<unsigned long long*>(ctx->scratch(TDX_S_M, size_t(tilek::COUNT_RING) * 16));
    DaPartial* partial = static_cast<DaPartial*>(ctx->scratch(TDX_S_D, size_t(nparts) * sizeof(DaPartial)));
    DaPartial* totals = static_cast<DaPartial*>(ctx->scratch(TDX_S_E, size_t(nthresh) * sizeof(DaPartial)));
    uint32_t* rowcnt = static_cast<uint32_t*>(ctx->scratch(TDX_S_F, size_t(nthresh) * 3 * size_t(iny) * 4));
    int32_t* d_out = static_cast<int32_t*>(ctx->scratch(TDX_S_R, (nout ? nout : 1) * 16));   // x, y, term, flag
    if (!info || !rec || !counts || !partial || !totals || !rowcnt || !d_out) return TDX_ERR_NOMEM;

    ctx->begin_call(stats);
    strip_mark(ctx, st, "dropanalysis");
    // the neighbours' boundary rows of the three inputs the sweeps read (src/DropAnalysis.cpp:361-363)
    int rc = strip_exchange<int16_t>(ctx, st, d_p, p_nodata);
    if (rc != TDX_OK) return rc;
    rc = strip_exchange<float>(ctx, st, d_ssa, ssa_nodata);
    if (rc != TDX_OK) return rc;
    rc = strip_exchange<float>(ctx, st, d_fel, DA_ELEV_NODATA);
    if (rc != TDX_OK) return rc;

    // ---- total area
    std::vector<int32_t> flag(nout, 0);
    if (nout) {
        TdxSpan sp(ctx, TDX_K_MISC);
        float* d_term = reinterpret_cast<float*>(d_out + 2 * nout);
        int32_t* d_flag = d_out + 3 * nout;
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_out, outlet_x, nout * 4, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_out + nout, outlet_y, nout * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(da_outlet_kernel, dim3(tdx_blocks_for(nout, 256)), dim3(256), 0, s, d_out, d_out + nout, int(nout), inx, iny, st.y0, st.y1, d_ad8, d_p, p_nodata,
                           d_ssa, ssa_nodata, d_term, d_flag);
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(outlet_term, d_term, nout * 4, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(flag.data(), d_flag, nout * 4, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
        if (stats) stats->launches[TDX_K_MISC]++;
        for (size_t i = 0; i < nout; i++)
            if (flag[i] == 2) {
                char msg[160];
                snprintf(msg, sizeof msg, "tdx_dropanalysis: outlet %zu (column %d, row %d) lies on a cell without a flow direction", i, int(outlet_x[i]), int(outlet_y[i]));
                return tdx_fail(ctx, TDX_ERR_ARG, msg);
            }
    }

    // ---- one sweep and one statistics pass per threshold
    TDX_HIP_CHECK(ctx, hipMemsetAsync(rowcnt, 0, size_t(nthresh) * 3 * size_t(iny) * 4, s));
    int64_t rounds = 0, launches = 0, outer = 0;
    for (int64_t th = 0; th < nthresh; th++) {
        const float thresh = dropan::ladder(thresh_min, thresh_max, int(nthresh), steptype, int(th));
        res.thresh[th] = thresh;
        {
            TdxSpan sp(ctx, TDX_K_STENCIL);
            hipLaunchKernelGGL(da_setup_kernel, grid2d, dim3(256), 0, s, d_p, d_ssa, inx, iny, p_nodata, ssa_nodata, thresh, info);
            hipLaunchKernelGGL(da_init_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, info, first, nown, rec);
            if (stats) stats->launches[TDX_K_STENCIL] += 2;
        }
        {
            const float2 oc = DropAlg::outside();
            uint2 ob;
            memcpy(&ob, &oc, sizeof(ob));
            rc = strip_exchange<uint2>(ctx, st, reinterpret_cast<uint2*>(rec), ob);
            if (rc != TDX_OK) return rc;
        }
        {
            TdxSpan sp(ctx, TDX_K_ACCUM);
            d8sweep::Arrays<DropAlg> A{rec, d_fel, nullptr, nullptr, info};
            int64_t o1 = 1;
            rc = d8sweep::run(ctx, st, DropAlg{}, A, counts, &rounds, &launches, &o1);
            if (rc != TDX_OK) return rc;
            outer += o1;
        }
        {
            TdxSpan sp(ctx, TDX_K_MISC);
            hipLaunchKernelGGL(da_stats_kernel, grid_stats, dim3(256), 0, s, rec, info, d_fel, inx, st.y0, st.y1, rowcnt + size_t(th) * 3 * size_t(iny), partial);
            hipLaunchKernelGGL(da_reduce_kernel, dim3(1), dim3(256), 0, s, partial, nparts, totals + th);
            if (stats) stats->launches[TDX_K_MISC] += 2;
            if (th == grid_th && (d_order || d_elev)) {
                hipLaunchKernelGGL(da_grids_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, rec, first, nown, d_order, d_elev);
                if (stats) stats->launches[TDX_K_MISC]++;
            }
        }
    }
    if (stats) stats->launches[TDX_K_ACCUM] += launches;
    TDX_HIP_CHECK(ctx, hipGetLastError());
    std::vector<DaPartial> tot(static_cast<size_t>(nthresh));
    std::vector<uint32_t> rows(size_t(nthresh) * 3 * size_t(iny));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(tot.data(), totals, tot.size() * sizeof(DaPartial), hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(rows.data(), rowcnt, rows.size() * 4, hipMemcpyDeviceToHost, s));
    tdx_stats* stt = stats;
    ctx->end_call();   // synchronises
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    for (int64_t th = 0; th < nthresh; th++) {
        const DaPartial& t = tot[size_t(th)];
        res.n1[th] = t.n[0];
        res.n2[th] = t.n[1];
        for (int i = 0; i < 4; i++) res.sums[4 * th + i] = t.s[i];
        // the links of a row times the row's cell sizes, rows top to bottom (src/DropAnalysis.cpp:498-501: dxc / dyc of the receiving cell's row)
        const uint32_t* rc3 = rows.data() + size_t(th) * 3 * size_t(iny);
        double length = 0.0;
        for (int y = st.y0; y < st.y1; y++) {
            const double dx = dxc[y], dy = dyc[y];
            if (rc3[3 * y + 0]) length = length + double(rc3[3 * y + 0]) * dx;
            if (rc3[3 * y + 1]) length = length + double(rc3[3 * y + 1]) * dy;
            if (rc3[3 * y + 2]) length = length + double(rc3[3 * y + 2]) * sqrt(dx * dx + dy * dy);
        }
        res.length[th] = length;
    }
    return TDX_OK;
}

int dropan_check(tdx_context* ctx, const void* ad8, const void* p, const void* fel, const void* ssa, const void* dxc, const void* dyc, int64_t nx, int64_t ny, int64_t halo,
                 const int32_t* outlet_x, const int32_t* outlet_y, int64_t n_outlets, const void* thresh, const void* n1, const void* n2, const void* sums, const void* length,
                 const char* who) {
    if (!ctx || !ad8 || !p || !fel || !ssa || !dxc || !dyc || !thresh || !n1 || !n2 || !sums || !length || nx <= 0 || ny <= 0)
        return tdx_fail(ctx, TDX_ERR_ARG, std::string(who) + ": bad argument");
    if (too_big(nx, ny + halo)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    if (n_outlets < 0 || (n_outlets > 0 && (!outlet_x || !outlet_y))) return tdx_fail(ctx, TDX_ERR_ARG, std::string(who) + ": outlets missing");
    return TDX_OK;
}
int dropan_check_ladder(tdx_context* ctx, int64_t nthresh) {
    if (nthresh < 2) return tdx_fail(ctx, TDX_ERR_ARG, "Number of thresholds must be greater than 1.");   // src/DropAnalysis.cpp:369-373
    if (nthresh > 100000) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_dropanalysis: more than 100000 thresholds");
    return TDX_OK;
}

// total area and optimum of a whole raster from the sums of dropan_impl (src/DropAnalysis.cpp:313-331, 597-644)
int dropan_finish(const DaResult& res, int64_t nthresh, const float* outlet_term, int64_t n_outlets, double dxA, double dyA, float* total_area, float* optimum,
                  int32_t* found, char* table, int64_t table_cap) {
    float ta = 0.f;
    for (int64_t i = 0; i < n_outlets; i++) ta += outlet_term[i];   // file order; a skipped outlet adds 0
    const float total = ta * dxA * dyA;
    std::vector<float> f(size_t(nthresh) * 4);
    for (int64_t th = 0; th < nthresh; th++)
        for (int i = 0; i < 4; i++) f[size_t(i) * size_t(nthresh) + size_t(th)] = float(res.sums[4 * th + i]);
    const size_t nt = size_t(nthresh);
    const dropan::Sums sm{nthresh, res.thresh, res.n1, res.n2, f.data(), f.data() + nt, f.data() + 2 * nt, f.data() + 3 * nt, res.length, total};
    float opt = 0.f;
    int fnd = 0;
    std::string tab;
    dropan::table(sm, table ? &tab : nullptr, nullptr, &opt, &fnd);
    if (table && int64_t(tab.size()) + 1 > table_cap) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_dropanalysis: table buffer too small");
    if (table) memcpy(table, tab.c_str(), tab.size() + 1);
    if (total_area) *total_area = total;
    if (optimum) *optimum = opt;
    if (found) *found = fnd;
    return TDX_OK;
}
}  // namespace

extern "C" int tdx_dropanalysis_dev(tdx_context* ctx, const float* d_ad8, const int16_t* d_p, const float* d_fel, const float* d_ssa, int64_t nx, int64_t ny,
                                    int16_t p_nodata, float ssa_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const int32_t* outlet_x,
                                    const int32_t* outlet_y, int64_t n_outlets, float thresh_min, float thresh_max, int64_t nthresh, int steptype, int64_t grid_th,
                                    int16_t* d_order, float* d_elevout, float* thresh, int64_t* n1, int64_t* n2, double* sums, double* length, float* total_area,
                                    float* optimum, int32_t* found, char* table, int64_t table_cap, tdx_stats* stats) {
    if (int rc = dropan_check(ctx, d_ad8, d_p, d_fel, d_ssa, dxc, dyc, nx, ny, 0, outlet_x, outlet_y, n_outlets, thresh, n1, n2, sums, length, "tdx_dropanalysis_dev")) return rc;
    if (int rc = dropan_check_ladder(ctx, nthresh)) return rc;
    const DaResult res{thresh, n1, n2, sums, length};
    std::vector<float> term(size_t(n_outlets), 0.f);
    const int rc = dropan_impl(ctx, strip_single(int(nx), int(ny)), d_ad8, const_cast<int16_t*>(d_p), p_nodata, const_cast<float*>(d_fel), const_cast<float*>(d_ssa), ssa_nodata,
                               dxc, dyc, outlet_x, outlet_y, n_outlets, thresh_min, thresh_max, nthresh, steptype, grid_th, d_order, d_elevout, res, term.data(), stats);
    if (rc != TDX_OK) return rc;
    return dropan_finish(res, nthresh, term.data(), n_outlets, dxA, dyA, total_area, optimum, found, table, table_cap);
}

extern "C" int tdx_dropanalysis(tdx_context* ctx, const float* ad8, const int16_t* p, const float* fel, const float* ssa, int64_t nx, int64_t ny, int16_t p_nodata,
                                float ssa_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const int32_t* outlet_x, const int32_t* outlet_y,
                                int64_t n_outlets, float thresh_min, float thresh_max, int64_t nthresh, int steptype, int64_t grid_th, int16_t* order, float* elevout,
                                float* thresh, int64_t* n1, int64_t* n2, double* sums, double* length, float* total_area, float* optimum, int32_t* found,
                                char* table, int64_t table_cap, tdx_stats* stats) {
    if (int rc = dropan_check(ctx, ad8, p, fel, ssa, dxc, dyc, nx, ny, 0, outlet_x, outlet_y, n_outlets, thresh, n1, n2, sums, length, "tdx_dropanalysis")) return rc;
    if (int rc = dropan_check_ladder(ctx, nthresh)) return rc;
    HostCall h(ctx, nx, ny);
    int16_t* d_p = h.in(TDX_S_IO0, p);
    float* d_fel = h.in(TDX_S_IO1, fel);
    float* d_ssa = h.in(TDX_S_IO2, ssa);
    float* d_ad8 = h.in(TDX_S_IO3, ad8);
    int16_t* d_o = h.out(TDX_S_IO4, order);    // optional
    float* d_e = h.out(TDX_S_N, elevout);      // optional
    if (h.error) return h.error;
    return h.finish(tdx_dropanalysis_dev(ctx, d_ad8, d_p, d_fel, d_ssa, nx, ny, p_nodata, ssa_nodata, dxc, dyc, dxA, dyA, outlet_x, outlet_y, n_outlets, thresh_min, thresh_max,
                                         nthresh, steptype, grid_th, d_o, d_e, thresh, n1, n2, sums, length, total_area, optimum, found, table, table_cap, stats));
}

// The strip's own counts, sums and length, and its outlets' terms of the total area (0 for an outlet of another strip): the caller adds the strips'
// n1 / n2 / sums / length in strip order and the outlet terms in file order, and makes the table with tdx_dropanalysis_table.
extern "C" int tdx_dropanalysis_strip(tdx_context* ctx, const tdx_comm* comm, const float* d_ad8, int16_t* d_p, float* d_fel, float* d_ssa, int64_t nx, int64_t ny_local,
                                      int16_t p_nodata, float ssa_nodata, const double* dxc, const double* dyc, const int32_t* outlet_x, const int32_t* outlet_row,
                                      int64_t n_outlets, float thresh_min, float thresh_max, int64_t nthresh, int steptype, int64_t grid_th, int16_t* d_order,
                                      float* d_elevout, float* thresh, int64_t* n1, int64_t* n2, double* sums, double* length, float* outlet_term, tdx_stats* stats) {
    if (int rc = dropan_check(ctx, d_ad8, d_p, d_fel, d_ssa, dxc, dyc, nx, ny_local, 2, outlet_x, outlet_row, n_outlets, thresh, n1, n2, sums, length, "tdx_dropanalysis_strip"))
        return rc;
    if (n_outlets > 0 && !outlet_term) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_dropanalysis_strip: bad argument");
    if (int rc = dropan_check_ladder(ctx, nthresh)) return rc;
    const DaResult res{thresh, n1, n2, sums, length};
    return dropan_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_ad8, d_p, p_nodata, d_fel, d_ssa, ssa_nodata, dxc, dyc, outlet_x, outlet_row, n_outlets, thresh_min,
                       thresh_max, nthresh, steptype, grid_th, d_order, d_elevout, res, outlet_term, stats);
}

extern "C" int tdx_dropanalysis_table(int64_t nthresh, const float* thresh, const int64_t* n1, const int64_t* n2, const float* s1, const float* s1sq, const float* s2,
                                      const float* s2sq, const double* length, float total_area, char* table, int64_t table_cap, char* console, int64_t console_cap,
                                      float* optimum, int32_t* found) {
    if (nthresh < 0 || (nthresh > 0 && (!thresh || !n1 || !n2 || !s1 || !s1sq || !s2 || !s2sq || !length)))
        return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_dropanalysis_table: bad argument");
    const dropan::Sums sm{nthresh, thresh, n1, n2, s1, s1sq, s2, s2sq, length, total_area};
    std::string tab, con;
    float opt = 0.f;
    int fnd = 0;
    dropan::table(sm, &tab, &con, &opt, &fnd);
    if ((table && int64_t(tab.size()) + 1 > table_cap) || (console && int64_t(con.size()) + 1 > console_cap))
        return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_dropanalysis_table: text buffer too small");
    if (table) memcpy(table, tab.c_str(), tab.size() + 1);
    if (console) memcpy(console, con.c_str(), con.size() + 1);
    if (optimum) *optimum = opt;
    if (found) *found = fnd;
    return TDX_OK;
}
