// DinfDistUp (dinfdistup, src/DinfDistUp.cpp) on gfx950: the distance from every cell up to the ridge along the D-infinity flow, in the
// four forms of the reference - horizontal (h, hdisttoridgegrd), vertical rise (v, vrisetoridgegrd), Pythagorean (p, pdisttoridgegrd) and
// surface (s, sdisttoridgegrd) - each as the average, maximum or minimum over the contributing neighbours, with the proportion threshold.
//
// The dependency shape is AreaDinf's (initNeighborDinfup without outlets): a cell waits for the neighbours whose flow reaches it and
// releases its at most two receivers, so it runs on the forward tile sweep of DinfConcLimAccum with the set-up of dinf_fwd.hpp.  A cell
// takes from each contributor its result, its angle (the proportion is the contributor's, with the contributor's row), its elevation
// and its weight, so all four travel in the contributor's 16-byte record {du, angle, fel, wt}; a cell's own elevation is the third slot
// of its own record.  The receiving cell's dist[j][k] comes from the engine's per-row table (HAS_DIST: the row of the evaluated cell).
// What the reference does per cell, in its float / double arithmetic:
//   * a neighbour off the raster or without an angle contaminates (INFO_CON of the set-up), whether it contributes or not;
//   * a contributor counts only if p > 0 and p > thresh (double); one with 0 < p <= thresh is waited for but otherwise ignored;
//   * a contributor without a result - or, for v / p / s, with a nodata elevation - contaminates and is skipped; otherwise
//     sump += p, and a nodata weight contaminates but the contributor still counts with wt = 1;
//   * step h: dist[j][k] * wt, v: elvn - elv (no weight), s: sqrtf((elv - elvn)^2 + (dist[j][k] * wt)^2); `acc = acc + p * (step + d)`
//     in double, rounded to float at every step; `ave` divides by the float sump once if sump > 0;
//   * `max h` starts from 0, every other max / min from the first counted contributor;
//   * p and s give nodata where the cell's own elevation is nodata; v does not test it and computes with the raw nodata value.
// p is two sweeps over the same info words, each with the same 16-byte record: the h part (with p's elevation tests and `first` under
// max) and the v part (with p's own-elevation test and weight contamination); the reference's finishing pass sqrt(h*h + v*v) is the
// unpack.  The two parts have the same contributors and the same nodata cells, so the split changes no bit.
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "context.hpp"
#include "d8_sweep.hpp"
#include "device_common.hpp"
#include "dinf_fwd.hpp"
#include "dinf_prop.hpp"

namespace {
using namespace tdxk;
using namespace dinffwd;

constexpr int KIND_H = 0, KIND_V = 1, KIND_P = 2, KIND_S = 3;
constexpr int PART_H = 4, PART_V = 5;   // the two sweeps of p
constexpr int STAT_AVE = 0, STAT_MAX = 1, STAT_MIN = 2;

// one statistic step over a contributor's candidate `x` (src/DinfDistUp.cpp:243-260 and its three siblings)
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

// record = {du, angle, fel, wt}.  KIND: KIND_H, KIND_V, KIND_S, PART_H or PART_V.  FIRST = false only for `max h` (src/DinfDistUp.cpp:248-249).
template <int KIND, int STAT, bool FIRST>
struct DistUpAlg {
    using Cell = float4;
    using Aux = float;   // (unused: the cell's own elevation is in its record)
    static constexpr bool HAS_AUX = false, HAS_DIST = true, HAS_ROWS = true;
    static constexpr int kBulkSweeps = 6;   // (DinfConcLimAccum's, same graph and record size)
    static constexpr unsigned kBulkUntil = 16;
    static constexpr int kMinWaves32 = 4;
    static constexpr int kMaxRelease = 2;
    static constexpr bool STEP_H = KIND == KIND_H || KIND == PART_H, STEP_V = KIND == KIND_V || KIND == PART_V;
    static constexpr bool FEL_GATE = KIND != KIND_H;                    // a contributor with a nodata elevation is skipped (v, p, s)
    static constexpr bool OWN_GATE = KIND != KIND_H && KIND != KIND_V;   // a nodata own elevation gives nodata (p, s; not v)
    static constexpr bool USE_W = KIND != KIND_V;                       // v reads no weights (p's v part does: a nodata weight contaminates)
    float fel_nodata, w_nodata;
    double thresh;
    int usew, concheck;
    static __device__ __forceinline__ float head(const float4& c) { return c.x; }
    static __host__ __device__ __forceinline__ float4 outside() { return make_float4(TDX_ANG_NODATA, TDX_ANG_NODATA, TDX_ANG_NODATA, TDX_ANG_NODATA); }
    static __device__ __forceinline__ unsigned rel_mask(unsigned inf) { return fwd_rel_mask(inf); }
    template <class L>
    __device__ __forceinline__ void eval(L& S, int c, int cl, int ly, unsigned inf, const Cell (&nb)[9]) const {
        float4 me = S.v[cl];
        const float elv = me.z;
        float res = TDX_ANG_NODATA;
        if (!(OWN_GATE && is_nodata_f(elv, fel_nodata))) {
            bool con = (inf & d8sweep::INFO_CON) != 0u, first = true;
            float acc = 0.0f, sump = 0.0f;
#pragma unroll
            for (int k = 1; k <= 8; k++) {
                if (!((inf >> (k - 1)) & 1u)) continue;
                const float4 n = nb[k];
                const double p = prop_dev(n.y, (k + 4) % 8, S.rows[ly + 1 + d2(k)]);   // the contributor's row
                if (!(p > 0. && p > thresh)) continue;
                if (is_nodata_f(n.x, TDX_ANG_NODATA)) { con = true; continue; }
                if (FEL_GATE && is_nodata_f(n.z, fel_nodata)) { con = true; continue; }
                sump = (float)((double)sump + p);
                float wt = 1.f;
                if (USE_W && usew) {
                    if (is_nodata_f(n.w, w_nodata)) con = true;
                    else wt = n.w;
                }
                float x;
                if (STEP_H) x = S.dist[ly * 9 + k] * wt + n.x;   // dist[j][k]: the row of the evaluated cell
                else if (STEP_V) x = (n.z - elv) + n.x;
                else {
                    const float dk = S.dist[ly * 9 + k] * wt, dz = elv - n.z;
                    x = sqrtf(dz * dz + dk * dk) + n.x;
                }
                fold<STAT, FIRST>(acc, first, p, x);
            }
            if (con && concheck) res = TDX_ANG_NODATA;
            else res = (STAT == STAT_AVE && sump > 0.f) ? acc / sump : acc;
        }
        me.x = res;
        S.v[cl] = me;
    }
};

// records of the owned rows: pending where the cell participates, "no value" elsewhere (never read: such a cell is nobody's contributor)
__global__ __launch_bounds__(256) void du_pack_kernel(const uint32_t* __restrict__ info, const float* __restrict__ ANG, const float* __restrict__ FEL,
                                                      const float* __restrict__ W, size_t first, size_t n, float4* __restrict__ rec) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    rec[i] = make_float4((info[i] & d8sweep::INFO_PART) ? __uint_as_float(d8sweep::PENDING_BITS) : TDX_ANG_NODATA, ANG[i], FEL ? FEL[i] : 0.f, W ? W[i] : 1.f);
}
// h / v / s, and the h part of p on its way to du_unpack_p_kernel: pending (on or below a cycle: never queued by the reference either) is nodata
__global__ __launch_bounds__(256) void du_unpack_kernel(const float4* __restrict__ rec, size_t first, size_t n, float* __restrict__ du) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    const float r = rec[i].x;
    du[i] = d8sweep::pending(r) ? TDX_ANG_NODATA : r;
}
// p: the finishing pass of pdisttoridgegrd (src/DinfDistUp.cpp:870-881): nodata where v is, else sqrt(h*h + v*v) in float; du holds h
__global__ __launch_bounds__(256) void du_unpack_p_kernel(const float4* __restrict__ rec, size_t first, size_t n, float* __restrict__ du) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    const float v = rec[i].x, h = du[i];
    float out;
    if (d8sweep::pending(v) || is_nodata_f(v, TDX_ANG_NODATA)) out = TDX_ANG_NODATA;
    else if (!is_nodata_f(h, TDX_ANG_NODATA)) out = sqrtf(h * h + v * v);
    else out = h;
    du[i] = out;
}

struct DuArgs {
    float* d_ang; float ang_nodata;
    const double* dxc; const double* dyc;
    const float* d_fel; float fel_nodata;
    const float* d_w; float w_nodata;
    int stat, kind, concheck;
    float thresh;
    float* d_du;
};

// packs the records of the owned rows and runs one sweep of policy Alg
template <class Alg>
int du_sweep(tdx_context* ctx, const Strip& st, const DuArgs& a, FwdSetup& R, const float* d_dist, tdx_stats* stats, int64_t* rounds, int64_t* outer) {
    hipStream_t s = ctx->stream;
    const size_t first = size_t(st.y0) * size_t(st.nx), nown = size_t(st.y1 - st.y0) * size_t(st.nx);
    const bool use_w = a.d_w != nullptr && a.kind != KIND_V;   // (v: the weight code is commented out in the reference)
    hipLaunchKernelGGL(du_pack_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.info, R.ang_use, a.kind != KIND_H ? a.d_fel : nullptr,
                       use_w ? a.d_w : nullptr, first, nown, R.rec);
    const Alg alg{a.fel_nodata, a.w_nodata, (double)a.thresh, use_w ? 1 : 0, a.concheck ? 1 : 0};   // (thresh: a float promoted to double)
    return fwd_sweep(ctx, st, alg, R, nullptr, stats, rounds, outer, d_dist);
}

// the mode is a template argument: A is the policy of h / v / s or of p's h part, B that of p's v part (void for one sweep)
template <class A, class B>
int du_run(tdx_context* ctx, const Strip& st, const DuArgs& a, tdx_stats* stats) {
    hipStream_t s = ctx->stream;
    const int inx = st.nx, iny = st.ny_arr;
    const size_t first = size_t(st.y0) * size_t(inx), nown = size_t(st.y1 - st.y0) * size_t(inx);
    // dist[j][k] = sqrt(dxc^2 d1^2 + dyc^2 d2^2) in double, stored as float (src/DinfDistUp.cpp:147-154); d1 / d2 of src/commonLib.h
    static const int hd1[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1}, hd2[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
    std::vector<float> dist(size_t(iny) * 9, 0.f);
    for (int m = 0; m < iny; m++)
        for (int k = 1; k <= 8; k++)
            dist[size_t(m) * 9 + size_t(k)] = (float)sqrt(a.dxc[m] * a.dxc[m] * hd1[k] * hd1[k] + a.dyc[m] * a.dyc[m] * hd2[k] * hd2[k]);
    float* d_dist = static_cast<float*>(ctx->scratch(TDX_S_F, dist.size() * sizeof(float)));
    if (!d_dist) return TDX_ERR_NOMEM;
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_dist, dist.data(), dist.size() * sizeof(float), hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));   // `dist` is a local
    FwdSetup R;
    int rc = fwd_prepare(ctx, st, a.d_ang, a.ang_nodata, a.dxc, a.dyc, nullptr, nullptr, -1, R, stats, "dinfdistup");   // (no outlets)
    if (rc != TDX_OK) return rc;
    int64_t rounds = 0, outer = 1;
    rc = du_sweep<A>(ctx, st, a, R, d_dist, stats, &rounds, &outer);
    if (rc != TDX_OK) return rc;
    hipLaunchKernelGGL(du_unpack_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.rec, first, nown, a.d_du);
    if constexpr (!std::is_void<B>::value) {   // p: the v part, then sqrt(h*h + v*v) with the h part kept in d_du
        int64_t outer2 = 1;
        rc = du_sweep<B>(ctx, st, a, R, d_dist, stats, &rounds, &outer2);
        if (rc != TDX_OK) return rc;
        outer += outer2;
        hipLaunchKernelGGL(du_unpack_p_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.rec, first, nown, a.d_du);
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    return TDX_OK;
}

// (kind, stat) -> policies: no branch on the mode inside the sweep
int distup_impl(tdx_context* ctx, const Strip& st, const DuArgs& a, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    switch (a.kind * 3 + a.stat) {
    case KIND_H * 3 + STAT_AVE: return du_run<DistUpAlg<KIND_H, STAT_AVE, true>, void>(ctx, st, a, stats);
    case KIND_H * 3 + STAT_MAX: return du_run<DistUpAlg<KIND_H, STAT_MAX, false>, void>(ctx, st, a, stats);
    case KIND_H * 3 + STAT_MIN: return du_run<DistUpAlg<KIND_H, STAT_MIN, true>, void>(ctx, st, a, stats);
    case KIND_V * 3 + STAT_AVE: return du_run<DistUpAlg<KIND_V, STAT_AVE, true>, void>(ctx, st, a, stats);
    case KIND_V * 3 + STAT_MAX: return du_run<DistUpAlg<KIND_V, STAT_MAX, true>, void>(ctx, st, a, stats);
    case KIND_V * 3 + STAT_MIN: return du_run<DistUpAlg<KIND_V, STAT_MIN, true>, void>(ctx, st, a, stats);
    case KIND_S * 3 + STAT_AVE: return du_run<DistUpAlg<KIND_S, STAT_AVE, true>, void>(ctx, st, a, stats);
    case KIND_S * 3 + STAT_MAX: return du_run<DistUpAlg<KIND_S, STAT_MAX, true>, void>(ctx, st, a, stats);
    case KIND_S * 3 + STAT_MIN: return du_run<DistUpAlg<KIND_S, STAT_MIN, true>, void>(ctx, st, a, stats);
    case KIND_P * 3 + STAT_AVE: return du_run<DistUpAlg<PART_H, STAT_AVE, true>, DistUpAlg<PART_V, STAT_AVE, true>>(ctx, st, a, stats);
    case KIND_P * 3 + STAT_MAX: return du_run<DistUpAlg<PART_H, STAT_MAX, true>, DistUpAlg<PART_V, STAT_MAX, true>>(ctx, st, a, stats);
    case KIND_P * 3 + STAT_MIN: return du_run<DistUpAlg<PART_H, STAT_MIN, true>, DistUpAlg<PART_V, STAT_MIN, true>>(ctx, st, a, stats);
    }
    return tdx_fail(ctx, TDX_ERR_ARG, "dinfdistup: statmethod must be 0..2 and typemethod 0..3");
}

bool bad_mode(int stat, int kind) { return stat < 0 || stat > 2 || kind < 0 || kind > 3; }

}  // namespace

// the argument test of the _dev (halo 0) and _strip (halo 2: the strip's two halo rows) entry points
static int distup_check(tdx_context* ctx, const void* ang, const void* fel, const void* du, const void* dxc, const void* dyc, int64_t nx, int64_t ny, int64_t halo,
                        int statmethod, int typemethod, const char* who) {
    if (!ctx || !ang || !du || !dxc || !dyc || nx <= 0 || ny <= 0 || bad_mode(statmethod, typemethod) || (typemethod != KIND_H && !fel))
        return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}

extern "C" int tdx_dinfdistup_dev(tdx_context* ctx, const float* d_ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc,
                                  const float* d_fel, float fel_nodata, const float* d_w, float w_nodata, int statmethod, int typemethod, int contcheck,
                                  float thresh, float* d_du, tdx_stats* stats) {
    if (int rc = distup_check(ctx, d_ang, d_fel, d_du, dxc, dyc, nx, ny, 0, statmethod, typemethod, "tdx_dinfdistup_dev: bad argument")) return rc;
    const DuArgs a{const_cast<float*>(d_ang), ang_nodata, dxc, dyc, d_fel, fel_nodata, d_w, w_nodata, statmethod, typemethod, contcheck, thresh, d_du};
    return distup_impl(ctx, strip_single(int(nx), int(ny)), a, stats);
}
extern "C" int tdx_dinfdistup_strip(tdx_context* ctx, const tdx_comm* comm, float* d_ang, int64_t nx, int64_t ny_local, float ang_nodata, const double* dxc,
                                    const double* dyc, const float* d_fel, float fel_nodata, const float* d_w, float w_nodata, int statmethod, int typemethod,
                                    int contcheck, float thresh, float* d_du, tdx_stats* stats) {
    if (int rc = distup_check(ctx, d_ang, d_fel, d_du, dxc, dyc, nx, ny_local, 2, statmethod, typemethod, "tdx_dinfdistup_strip: bad argument")) return rc;
    const DuArgs a{d_ang, ang_nodata, dxc, dyc, d_fel, fel_nodata, d_w, w_nodata, statmethod, typemethod, contcheck, thresh, d_du};
    return distup_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), a, stats);
}
extern "C" int tdx_dinfdistup(tdx_context* ctx, const float* ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc, const float* fel,
                              float fel_nodata, const float* w, float w_nodata, int statmethod, int typemethod, int contcheck, float thresh, float* du,
                              tdx_stats* stats) {
    if (!ctx || !ang || !du || nx <= 0 || ny <= 0 || bad_mode(statmethod, typemethod) || (typemethod != KIND_H && !fel))
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_dinfdistup: bad argument");
    HostCall h(ctx, nx, ny);
    float* d_a = h.in(TDX_S_IO0, ang);
    float* d_f = h.in(TDX_S_IO1, typemethod != KIND_H ? fel : nullptr);   // the horizontal distance reads no elevations,
    float* d_w = h.in(TDX_S_IO2, typemethod != KIND_V ? w : nullptr);     // the vertical one no weights (optional anyway)
    float* d_o = h.out(TDX_S_IO4, du);
    if (h.error) return h.error;
    return h.finish(tdx_dinfdistup_dev(ctx, d_a, nx, ny, ang_nodata, dxc, dyc, d_f, fel_nodata, d_w, w_nodata, statmethod, typemethod, contcheck, thresh, d_o, stats));
}
