// DinfDistDown (dinfdistdown, src/DinfDistDown.cpp) on gfx950: the distance from every cell down to the stream along the D-infinity
// flow, in the four forms of the reference - horizontal (h, hdisttostreamgrd), vertical drop (v, vdroptostreamgrd: with `ave` this
// is HAND), Pythagorean (p, pdisttostreamgrd) and surface (s, sdisttostreamgrd) - each as the average, maximum or minimum over
// the receivers.
//
// The dependency shape is that of DinfRevAccum (dinfrev.hip): a cell waits for its at most two receivers and releases the
// neighbours that drain into it, so it runs on the reverse tile sweep (d8sweep::sweep_tile_rev) with the set-up of dinf_rev.hpp.
// What differs:
//   * stream cells (src >= 1 as a short, with an angle) have an empty dependency mask and evaluate to 0 (src/DinfDistDown.cpp:222-224,
//     254-257); info bit 25 marks them.  A stream cell without an angle is never queued and stays nodata.
//   * everything a cell takes from its receivers besides their results is STATIC - their elevation, their weight, the step dist[j][k] * wt
//     to them - so one set-up pass folds it into the cell's own input record (DistAux): the step to each receiver in the reference's
//     float arithmetic, and flags for "contaminated whatever the results" (a receiver with prop > 0 outside the raster or without an
//     angle, or with a nodata elevation / weight) and "this receiver is skipped" (nodata elevation: the branch before sump += p).  The
//     sweep then reads nothing but the receivers' records, as it does for DinfRevAccum.
//   * the arithmetic per cell is the reference's: float accumulators, double proportions, every `acc = acc + p * (step + d)` evaluated
//     in double and rounded to float, `ave` divided by the float sump once at the end.
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "context.hpp"
#include "d8_sweep.hpp"
#include "device_common.hpp"
#include "dinf_prop.hpp"
#include "dinf_rev.hpp"

namespace {
using namespace tdxk;
using namespace dinfrev;

constexpr unsigned DINFO_STREAM = 1u << 25;   // info word: the cell is a stream cell (bits 25-31 are free in d8_sweep.hpp and dinf_rev.hpp)
// DistAux flags (the last word of the record, as bits)
constexpr unsigned DF_STREAM = 1u, DF_NODATA = 2u, DF_CON = 4u, DF_SKIP0 = 8u;   // DF_SKIP0 << t: receiver t is skipped
constexpr int KIND_H = 0, KIND_V = 1, KIND_P = 2, KIND_S = 3;
constexpr int STAT_AVE = 0, STAT_MAX = 1, STAT_MIN = 2;

// per-cell input record of h / v / s: {angle, step to receiver 0, step to receiver 1, flags}; the receivers in ascending k (receivers())
using DistAux = float4;
// p: {angle, horizontal step 0, horizontal step 1, flags} and {vertical step 0, vertical step 1, -, -} (32 bytes, two 16-byte loads)
struct alignas(16) DistAuxP {
    float4 a;
    float4 b;
};

__device__ __forceinline__ unsigned aux_flags(const DistAux& a) { return __float_as_uint(a.w); }
__device__ __forceinline__ unsigned aux_flags(const DistAuxP& a) { return __float_as_uint(a.a.w); }

// Stream cells: empty dependency mask, info bit 25 (owned rows only: the halo rows of a strip hold no src values).  Then the static part of
// each participating cell's evaluation, in the reference's float arithmetic:
//   h: dist[j][k] * wt                             (src/DinfDistDown.cpp:284-297)
//   v: elv - elvn                                  (wt stays 1: the weight code is commented out there)
//   s: sqrt((elv - elvn)^2 + (dist[j][k] * wt)^2)  (all float operands; rounded to float)
//   p: both the h and the v step
// A receiver with a nodata weight contaminates but still counts with wt = 1 (sump was incremented before the weight is read).
template <int KIND>
__global__ __launch_bounds__(256) void dd_setup_kernel(int nx, int y_own0, int y_own1, const int16_t* __restrict__ src, const float* __restrict__ fel, float fel_nodata,
                                                       const float* __restrict__ w, float w_nodata, const float* __restrict__ ang, const float* __restrict__ dist,
                                                       uint32_t* __restrict__ info, typename std::conditional<KIND == KIND_P, DistAuxP, DistAux>::type* __restrict__ aux) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = y_own0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= nx || y >= y_own1) return;
    const size_t idx = size_t(y) * size_t(nx) + size_t(x);
    unsigned inf = info[idx];
    if (!(inf & d8sweep::INFO_PART)) return;   // (no angle: never queued, never read)
    unsigned fl = 0;
    float sh[2] = {0.f, 0.f}, sv[2] = {0.f, 0.f};
    if (src[idx] >= 1) {   // srcData->getData(i, j, tempShort) >= 1
        fl |= DF_STREAM;
        inf = (inf & ~0xFFu) | DINFO_STREAM;
        info[idx] = inf;
    } else {
        constexpr bool USE_FEL = KIND != KIND_H, USE_W = KIND != KIND_V;
        float elv = 0.f;
        if (USE_FEL) {
            elv = fel[idx];
            if (is_nodata_f(elv, fel_nodata)) fl |= DF_NODATA;
        }
        const Recv r = receivers(inf);
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (!r.on[t]) continue;                                   // prop <= 0: not a receiver
            const int k = r.k[t];
            if (!((inf >> (k - 1)) & 1u)) { fl |= DF_CON; continue; }   // outside the raster or without an angle: its result stays nodata
            const size_t in = size_t(y + d2(k)) * size_t(nx) + size_t(x + d1(k));
            if (USE_FEL) {
                const float elvn = fel[in];
                if (is_nodata_f(elvn, fel_nodata)) { fl |= DF_CON | (DF_SKIP0 << t); continue; }
                sv[t] = elv - elvn;
            }
            float wt = 1.f;
            if (USE_W && w) {
                const float wn = w[in];
                if (is_nodata_f(wn, w_nodata)) fl |= DF_CON;
                else wt = wn;
            }
            const float dk = dist[size_t(y) * 9 + size_t(k)] * wt;
            if (KIND == KIND_S) sh[t] = sqrtf(sv[t] * sv[t] + dk * dk);
            else sh[t] = dk;
        }
    }
    const float a = ang[idx];
    if constexpr (KIND == KIND_P) {
        aux[idx] = DistAuxP{make_float4(a, sh[0], sh[1], __uint_as_float(fl)), make_float4(sv[0], sv[1], 0.f, 0.f)};
    } else {
        const float s0 = KIND == KIND_V ? sv[0] : sh[0], s1 = KIND == KIND_V ? sv[1] : sh[1];
        aux[idx] = make_float4(a, s0, s1, __uint_as_float(fl));
    }
}

// one statistic step over a receiver's candidate `x` (src/DinfDistDown.cpp:284-297 and its three siblings)
template <int STAT, bool FIRST>
__device__ __forceinline__ void fold(float& acc, bool& first, double p, float x) {
    if (STAT == STAT_AVE) acc = (float)((double)acc + p * (double)x);
    else if (STAT == STAT_MAX) {
        if (FIRST && first) { acc = x; first = false; }
        else if (x > acc) acc = x;
    } else {
        if (first) { acc = x; first = false; }
        else if (x < acc) acc = x;
    }
}

// h / v / s: one float per cell.  FIRST = false only for `max h`, which starts from 0 instead of the first receiver (src/DinfDistDown.cpp:287-289).
template <int STAT, bool FIRST>
struct DistDownAlg {
    using Cell = float;
    using Aux = DistAux;
    static constexpr bool HAS_AUX = true, HAS_DIST = false, HAS_ROWS = true;
    static constexpr int kBulkSweeps = 0;            // (not used by sweep_tile_rev)
    static constexpr unsigned kBulkUntil = 64;
    static constexpr int kMinWaves32 = 4;
    static constexpr int kMaxRelease = 8;
    int concheck;
    static __device__ __forceinline__ float head(float c) { return c; }
    static __host__ __device__ __forceinline__ float outside() { return TDX_ANG_NODATA; }
    static __device__ __forceinline__ unsigned rel_mask(unsigned inf) { return (inf >> 16) & 0xFFu; }
    static __device__ __forceinline__ void rev_row(unsigned inf, const Aux& a, double a2, int (&k)[2], bool (&on)[2], double (&p)[2]) { rev_row_dinf(inf, a.x, a2, k, on, p); }
    __device__ __forceinline__ Cell eval2(const Aux& a, const bool (&on)[2], const double (&p)[2], const Cell (&n)[2]) const {
        const unsigned fl = aux_flags(a);
        if (fl & DF_STREAM) return 0.0f;
        if (fl & DF_NODATA) return TDX_ANG_NODATA;
        bool con = (fl & DF_CON) != 0u, first = true;
        float acc = 0.0f, sump = 0.0f;
        const float step[2] = {a.y, a.z};
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (!on[t]) continue;
            if (is_nodata_f(n[t], TDX_ANG_NODATA)) { con = true; continue; }
            if (fl & (DF_SKIP0 << t)) continue;   // nodata elevation there (DF_CON is set)
            sump = (float)((double)sump + p[t]);
            fold<STAT, FIRST>(acc, first, p[t], step[t] + n[t]);
        }
        if ((con && concheck) || sump <= 0.0f) return TDX_ANG_NODATA;
        return STAT == STAT_AVE ? acc / sump : acc;
    }
    template <class L>
    __device__ __forceinline__ void eval(L& S, int c, int cl, int ly, unsigned inf, const Cell (&nb)[9]) const {
        const Aux a = S.aux[c];
        int k[2];
        bool on[2];
        double p[2];
        rev_row(inf, a, S.rows[ly + 1], k, on, p);
        Cell n[2] = {0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int kk = 1; kk <= 8; kk++) if (kk == k[t]) n[t] = nb[kk];
        S.v[cl] = eval2(a, on, p, n);
    }
};

// p: {h, v} as one 8-byte record (one store, as DinfRevAccum's); both parts share sump and the contamination test, which reads h
// (src/DinfDistDown.cpp:897-941).  The Pythagorean sum is taken by dd_unpack_p_kernel.
template <int STAT>
struct DistDownPAlg {
    using Cell = float2;
    using Aux = DistAuxP;
    static constexpr bool HAS_AUX = true, HAS_DIST = false, HAS_ROWS = true;
    static constexpr int kBulkSweeps = 0;
    static constexpr unsigned kBulkUntil = 64;
    static constexpr int kMinWaves32 = 4;
    static constexpr int kMaxRelease = 8;
    int concheck;
    static __device__ __forceinline__ float head(const float2& c) { return c.x; }
    static __host__ __device__ __forceinline__ float2 outside() { return make_float2(TDX_ANG_NODATA, TDX_ANG_NODATA); }
    static __device__ __forceinline__ unsigned rel_mask(unsigned inf) { return (inf >> 16) & 0xFFu; }
    static __device__ __forceinline__ void rev_row(unsigned inf, const Aux& a, double a2, int (&k)[2], bool (&on)[2], double (&p)[2]) { rev_row_dinf(inf, a.a.x, a2, k, on, p); }
    __device__ __forceinline__ Cell eval2(const Aux& a, const bool (&on)[2], const double (&p)[2], const Cell (&n)[2]) const {
        const unsigned fl = aux_flags(a);
        if (fl & DF_STREAM) return make_float2(0.0f, 0.0f);
        if (fl & DF_NODATA) return make_float2(TDX_ANG_NODATA, TDX_ANG_NODATA);
        bool con = (fl & DF_CON) != 0u, fh = true, fv = true;
        float acch = 0.0f, accv = 0.0f, sump = 0.0f;
        const float sh[2] = {a.a.y, a.a.z}, sv[2] = {a.b.x, a.b.y};
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (!on[t]) continue;
            if (is_nodata_f(n[t].x, TDX_ANG_NODATA)) { con = true; continue; }
            if (fl & (DF_SKIP0 << t)) continue;
            sump = (float)((double)sump + p[t]);
            fold<STAT, true>(acch, fh, p[t], sh[t] + n[t].x);
            fold<STAT, true>(accv, fv, p[t], sv[t] + n[t].y);
        }
        if ((con && concheck) || sump <= 0.0f) return make_float2(TDX_ANG_NODATA, TDX_ANG_NODATA);
        return STAT == STAT_AVE ? make_float2(acch / sump, accv / sump) : make_float2(acch, accv);
    }
    template <class L>
    __device__ __forceinline__ void eval(L& S, int c, int cl, int ly, unsigned inf, const Cell (&nb)[9]) const {
        const Aux a = S.aux[c];
        int k[2];
        bool on[2];
        double p[2];
        rev_row(inf, a, S.rows[ly + 1], k, on, p);
        Cell n[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int kk = 1; kk <= 8; kk++) if (kk == k[t]) n[t] = nb[kk];
        S.v[cl] = eval2(a, on, p, n);
    }
};

// h / v / s: cells still pending (on or above a cycle: never queued by the reference either) become nodata
__global__ __launch_bounds__(256) void dd_unpack_kernel(const float* __restrict__ rec, size_t first, size_t n, float* __restrict__ dd) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    const float r = rec[i];
    dd[i] = d8sweep::pending(r) ? TDX_ANG_NODATA : r;
}
// p: the finishing pass of pdisttostreamgrd (src/DinfDistDown.cpp:1013-1025): nodata where v is, else sqrt(h*h + v*v) in float
__global__ __launch_bounds__(256) void dd_unpack_p_kernel(const float2* __restrict__ rec, size_t first, size_t n, float* __restrict__ dd) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    const float2 r = rec[i];
    float out;
    if (d8sweep::pending(r.x) || is_nodata_f(r.y, TDX_ANG_NODATA)) out = TDX_ANG_NODATA;
    else if (!is_nodata_f(r.x, TDX_ANG_NODATA)) out = sqrtf(r.x * r.x + r.y * r.y);
    else out = r.x;
    dd[i] = out;
}

struct DdArgs {
    float* d_ang; float ang_nodata;
    const double* dxc; const double* dyc;
    float* d_fel; float fel_nodata;
    const int16_t* d_src;
    float* d_w; float w_nodata;
    int stat, kind, concheck;
    float* d_dd;
};

template <class Alg, int KIND>
int dd_run(tdx_context* ctx, const Strip& st, const DdArgs& a, Alg alg, tdx_stats* stats) {
    using Aux = typename Alg::Aux;
    using Cell = typename Alg::Cell;
    hipStream_t s = ctx->stream;
    const int inx = st.nx, iny = st.ny_arr;
    const size_t n = size_t(inx) * size_t(iny);
    const size_t first = size_t(st.y0) * size_t(inx), nown = size_t(st.y1 - st.y0) * size_t(inx);
    // dist[j][k] = sqrt(dxc^2 d1^2 + dyc^2 d2^2) in double, stored as float (src/DinfDistDown.cpp:142-150); d1 / d2 of src/commonLib.h
    static const int hd1[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1}, hd2[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
    std::vector<float> dist(size_t(iny) * 9, 0.f);
    for (int m = 0; m < iny; m++)
        for (int k = 1; k <= 8; k++)
            dist[size_t(m) * 9 + size_t(k)] = (float)sqrt(a.dxc[m] * a.dxc[m] * hd1[k] * hd1[k] + a.dyc[m] * a.dyc[m] * hd2[k] * hd2[k]);
    float* d_dist = static_cast<float*>(ctx->scratch(TDX_S_F, dist.size() * sizeof(float)));
    Aux* aux = static_cast<Aux*>(ctx->scratch(TDX_S_E, n * sizeof(Aux)));
    Cell* rec = static_cast<Cell*>(ctx->scratch(TDX_S_C, n * sizeof(Cell)));
    if (!d_dist || !aux || !rec) return TDX_ERR_NOMEM;
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_dist, dist.data(), dist.size() * sizeof(float), hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));   // `dist` is a local
    RevSetup R;
    int rc = rev_prepare(ctx, st, a.d_ang, a.ang_nodata, a.dxc, a.dyc, R, stats, "dinfdistdown");
    if (rc != TDX_OK) return rc;
    // felData->share(), weightData->share(): the receivers of the edge rows lie in the neighbours' strips
    if (KIND != KIND_H) { rc = strip_exchange<float>(ctx, st, a.d_fel, a.fel_nodata); if (rc != TDX_OK) return rc; }
    if (KIND != KIND_V && a.d_w) { rc = strip_exchange<float>(ctx, st, a.d_w, a.w_nodata); if (rc != TDX_OK) return rc; }
    const int rows_own = st.y1 - st.y0;
    hipLaunchKernelGGL((dd_setup_kernel<KIND>), dim3((inx + 63) / 64, (rows_own + 3) / 4), dim3(256), 0, s, inx, st.y0, st.y1, a.d_src, a.d_fel, a.fel_nodata,
                       KIND == KIND_V ? nullptr : a.d_w, a.w_nodata, a.d_ang, d_dist, R.info, aux);
    if (stats) stats->launches[TDX_K_STENCIL]++;
    if constexpr (sizeof(Cell) == 8) {
        hipLaunchKernelGGL(rev_init2_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.info, reinterpret_cast<float2*>(rec), first, nown);
        const Cell oc = Alg::outside();
        uint2 ob;
        memcpy(&ob, &oc, sizeof(ob));
        rc = strip_exchange<uint2>(ctx, st, reinterpret_cast<uint2*>(rec), ob);
    } else {
        hipLaunchKernelGGL(d8sweep::init_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.info, reinterpret_cast<float*>(rec), first, nown, TDX_ANG_NODATA);
        rc = strip_exchange<float>(ctx, st, reinterpret_cast<float*>(rec), TDX_ANG_NODATA);
    }
    if (rc != TDX_OK) return rc;
    int64_t rounds = 0, launches = 0, outer = 1;
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        d8sweep::Arrays<Alg> A{rec, aux, nullptr, R.d_a2, R.info};
        rc = d8sweep::run(ctx, st, alg, A, R.counts, &rounds, &launches, &outer);
        if (rc != TDX_OK) return rc;
        if constexpr (sizeof(Cell) == 8)
            hipLaunchKernelGGL(dd_unpack_p_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, reinterpret_cast<const float2*>(rec), first, nown, a.d_dd);
        else
            hipLaunchKernelGGL(dd_unpack_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, reinterpret_cast<const float*>(rec), first, nown, a.d_dd);
        if (stats) stats->launches[TDX_K_ACCUM] += launches;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    return TDX_OK;
}

// (kind, stat) -> one policy: no branch on the mode inside the sweep
int distdown_impl(tdx_context* ctx, const Strip& st, const DdArgs& a, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int cc = a.concheck ? 1 : 0;
    switch (a.kind * 3 + a.stat) {
    case KIND_H * 3 + STAT_AVE: return dd_run<DistDownAlg<STAT_AVE, true>, KIND_H>(ctx, st, a, {cc}, stats);
    case KIND_H * 3 + STAT_MAX: return dd_run<DistDownAlg<STAT_MAX, false>, KIND_H>(ctx, st, a, {cc}, stats);
    case KIND_H * 3 + STAT_MIN: return dd_run<DistDownAlg<STAT_MIN, true>, KIND_H>(ctx, st, a, {cc}, stats);
    case KIND_V * 3 + STAT_AVE: return dd_run<DistDownAlg<STAT_AVE, true>, KIND_V>(ctx, st, a, {cc}, stats);
    case KIND_V * 3 + STAT_MAX: return dd_run<DistDownAlg<STAT_MAX, true>, KIND_V>(ctx, st, a, {cc}, stats);
    case KIND_V * 3 + STAT_MIN: return dd_run<DistDownAlg<STAT_MIN, true>, KIND_V>(ctx, st, a, {cc}, stats);
    case KIND_S * 3 + STAT_AVE: return dd_run<DistDownAlg<STAT_AVE, true>, KIND_S>(ctx, st, a, {cc}, stats);
    case KIND_S * 3 + STAT_MAX: return dd_run<DistDownAlg<STAT_MAX, true>, KIND_S>(ctx, st, a, {cc}, stats);
    case KIND_S * 3 + STAT_MIN: return dd_run<DistDownAlg<STAT_MIN, true>, KIND_S>(ctx, st, a, {cc}, stats);
    case KIND_P * 3 + STAT_AVE: return dd_run<DistDownPAlg<STAT_AVE>, KIND_P>(ctx, st, a, {cc}, stats);
    case KIND_P * 3 + STAT_MAX: return dd_run<DistDownPAlg<STAT_MAX>, KIND_P>(ctx, st, a, {cc}, stats);
    case KIND_P * 3 + STAT_MIN: return dd_run<DistDownPAlg<STAT_MIN>, KIND_P>(ctx, st, a, {cc}, stats);
    }
    return tdx_fail(ctx, TDX_ERR_ARG, "dinfdistdown: statmethod must be 0..2 and typemethod 0..3");
}

bool bad_mode(int stat, int kind) { return stat < 0 || stat > 2 || kind < 0 || kind > 3; }

}  // namespace

// the argument test of the _dev (halo 0) and _strip (halo 2: the strip's two halo rows) entry points
static int distdown_check(tdx_context* ctx, const void* ang, const void* fel, const void* src, const void* dd, const void* dxc, const void* dyc, int64_t nx, int64_t ny,
                          int64_t halo, int statmethod, int typemethod, const char* who) {
    if (!ctx || !ang || !src || !dd || !dxc || !dyc || nx <= 0 || ny <= 0 || bad_mode(statmethod, typemethod) || (typemethod != KIND_H && !fel))
        return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}

extern "C" int tdx_dinfdistdown_dev(tdx_context* ctx, const float* d_ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc,
                                    const float* d_fel, float fel_nodata, const int16_t* d_src, const float* d_w, float w_nodata, int statmethod, int typemethod,
                                    int contcheck, float* d_dd, tdx_stats* stats) {
    if (int rc = distdown_check(ctx, d_ang, d_fel, d_src, d_dd, dxc, dyc, nx, ny, 0, statmethod, typemethod, "tdx_dinfdistdown_dev: bad argument")) return rc;
    const DdArgs a{const_cast<float*>(d_ang), ang_nodata, dxc, dyc, const_cast<float*>(d_fel), fel_nodata, d_src, const_cast<float*>(d_w), w_nodata,
                   statmethod, typemethod, contcheck, d_dd};
    return distdown_impl(ctx, strip_single(int(nx), int(ny)), a, stats);
}
extern "C" int tdx_dinfdistdown_strip(tdx_context* ctx, const tdx_comm* comm, float* d_ang, int64_t nx, int64_t ny_local, float ang_nodata, const double* dxc,
                                      const double* dyc, float* d_fel, float fel_nodata, const int16_t* d_src, float* d_w, float w_nodata, int statmethod,
                                      int typemethod, int contcheck, float* d_dd, tdx_stats* stats) {
    if (int rc = distdown_check(ctx, d_ang, d_fel, d_src, d_dd, dxc, dyc, nx, ny_local, 2, statmethod, typemethod, "tdx_dinfdistdown_strip: bad argument")) return rc;
    const DdArgs a{d_ang, ang_nodata, dxc, dyc, d_fel, fel_nodata, d_src, d_w, w_nodata, statmethod, typemethod, contcheck, d_dd};
    return distdown_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), a, stats);
}
extern "C" int tdx_dinfdistdown(tdx_context* ctx, const float* ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc, const float* fel,
                                float fel_nodata, const int16_t* src, const float* w, float w_nodata, int statmethod, int typemethod, int contcheck, float* dd,
                                tdx_stats* stats) {
    if (!ctx || !ang || !src || !dd || nx <= 0 || ny <= 0 || bad_mode(statmethod, typemethod) || (typemethod != KIND_H && !fel))
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_dinfdistdown: bad argument");
    HostCall h(ctx, nx, ny);
    float* d_a = h.in(TDX_S_IO0, ang);
    float* d_f = h.in(TDX_S_IO1, typemethod != KIND_H ? fel : nullptr);   // the horizontal distance reads no elevations,
    float* d_w = h.in(TDX_S_IO2, typemethod != KIND_V ? w : nullptr);     // the vertical one no weights (optional anyway)
    int16_t* d_s = h.in(TDX_S_IO3, src);
    float* d_o = h.out(TDX_S_IO4, dd);
    if (h.error) return h.error;
    return h.finish(tdx_dinfdistdown_dev(ctx, d_a, nx, ny, ang_nodata, dxc, dyc, d_f, fel_nodata, d_s, d_w, w_nodata, statmethod, typemethod, contcheck, d_o, stats));
}
